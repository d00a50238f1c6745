// Matrices from arrays in device memory.  In: rp.i32, ci.i32, val.f64 (a CSR matrix, rows = cols), trow.i32, tcol.i32, tval.f64, tval2.f64
// (unordered triples with duplicates, and other values for them), A.mtx and A2.mtx (one pattern, two sets of values).
#include "face_io.hpp"
using namespace mgs;

int main(int argc, char **argv) {
  return face::run(argc, argv, [](const std::string &in, face::Out &out) {
    const std::vector<int32_t> rp = face::read_raw<int32_t>(in + "rp.i32"), ci = face::read_raw<int32_t>(in + "ci.i32"),
                               trow = face::read_raw<int32_t>(in + "trow.i32"), tcol = face::read_raw<int32_t>(in + "tcol.i32");
    const int n = (int)rp.size() - 1;
    Vector val = face::load_vec(in + "val.f64"), tval = face::load_vec(in + "tval.f64"), tval2 = face::load_vec(in + "tval2.f64");
    {
      face::DevList<int32_t> drp(rp), dci(ci);
      out.csr("from_device32", DeviceMatrix::fromDevice(n, n, (int64_t)ci.size(), drp.ptr(), dci.ptr(), 32, mgs_vec_ptr(val.handle())));
    }
    {
      face::DevList<int64_t> drp(face::widen(rp)), dci(face::widen(ci));
      out.csr("from_device64", DeviceMatrix::fromDevice(n, n, (int64_t)ci.size(), drp.ptr(), dci.ptr(), 64, mgs_vec_ptr(val.handle())));
    }
    {
      face::DevList<int32_t> dr(trow), dc(tcol);
      DeviceMatrix T = DeviceMatrix::fromCooDevice(n, n + 3, dr.n, dr.ptr(), dc.ptr(), 32, mgs_vec_ptr(tval.handle()));
      out.csr("from_coo32", T);
    }
    {
      face::DevList<int64_t> dr(face::widen(trow)), dc(face::widen(tcol));
      DeviceMatrix T = DeviceMatrix::fromCooDevice(n, n + 3, dr.n, dr.ptr(), dc.ptr(), 64, mgs_vec_ptr(tval.handle()), true);
      out.csr("from_coo64_kept", T);
      T.update_values_coo(mgs_vec_ptr(tval2.handle()), tval2.size());
      out.csr("update_values_coo", T);
      Vector x(n + 3); x.upload(std::vector<double>((size_t)n + 3, 1.0));
      out.vec("coo_row_sums", T * x);
    }
    {
      const SMatrix A = readMatrix(in + "A.mtx"), A2 = readMatrix(in + "A2.mtx");
      DeviceMatrix Ad(A), shared = Ad;                                  // copies share the device matrix
      Ad.update_values(A2);
      out.csr("update_values", shared);
      writeMatrix(out.dir + "/A2_written.mtx", A2);                      // host only: the file the Python face writes from the same arrays
      out.count("written.nonzeros", A2.nonZeros());
    }
  });
}
