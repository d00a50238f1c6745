// Matrix algebra of mgs::DeviceMatrix, Vector::gather / scatter.  In: R.mtx (square), B.mtx (rectangular, R.cols rows), R2.mtx / B2.mtx
// (their patterns, other values), dl.f64, dr.f64, dlB.f64, drB.f64, x.f64, index lists rows.i32, cols.i32, rperm.i32, cperm.i32, gidx.i32.
#include "face_io.hpp"
using namespace mgs;
typedef face::DevList<int32_t> L32;
typedef face::DevList<int64_t> L64;

int main(int argc, char **argv) {
  return face::run(argc, argv, [](const std::string &in, face::Out &out) {
    const SMatrix hR = readMatrix(in + "R.mtx"), hB = readMatrix(in + "B.mtx"), hR2 = readMatrix(in + "R2.mtx"), hB2 = readMatrix(in + "B2.mtx");
    DeviceMatrix R(hR), B(hB);
    const std::vector<int32_t> rows = face::read_raw<int32_t>(in + "rows.i32"), cols = face::read_raw<int32_t>(in + "cols.i32"),
                               rperm = face::read_raw<int32_t>(in + "rperm.i32"), cperm = face::read_raw<int32_t>(in + "cperm.i32"),
                               gidx = face::read_raw<int32_t>(in + "gidx.i32");
    L32 rows32(rows), cols32(cols), rperm32(rperm), cperm32(cperm), gidx32(gidx);
    L64 rows64(face::widen(rows)), cols64(face::widen(cols)), cperm64(face::widen(cperm)), gidx64(face::widen(gidx));
    int64_t misses = -7;

    // ---- built from the first values
    DeviceMatrix C = R.multiply(B);                                     // rectangular: rows of R, columns of B
    out.csr("multiply", C);
    DeviceMatrix Rt = R.transpose(), Bt = B.transpose();
    out.csr("transpose", Bt); out.csr("transpose_square", Rt);
    DeviceMatrix S = R.add(Rt, 2.5, -0.75);
    out.csr("add", S);
    out.csr("add_default", R.add(Rt));
    out.vec("diagonal", B.diagonal());                                  // min(rows, cols) entries, one of them a stored zero
    out.vec("diagonal_t", Bt.diagonal());
    out.csr("from_diagonal", DeviceMatrix::fromDiagonal(B.diagonal()));
    DeviceMatrix Er = R.extract(rows32.ptr(), rows32.n, nullptr, 0, 32);             // repeated rows, every column
    DeviceMatrix Ec = B.extract(nullptr, 0, cols32.ptr(), cols32.n, 32);             // every row of the rectangular matrix
    DeviceMatrix Eb = R.extract(rows64.ptr(), rows64.n, cols64.ptr(), cols64.n, 64, true);
    DeviceMatrix Ea = B.extract(nullptr, 5, nullptr, 7);                             // lengths of NULL lists are ignored
    out.csr("extract_rows", Er); out.csr("extract_cols", Ec); out.csr("extract_both64", Eb); out.csr("extract_all", Ea);
    DeviceMatrix Pm = R.permute(rperm32.ptr(), cperm32.ptr(), 32, true);
    DeviceMatrix Pc = R.permute(nullptr, cperm64.ptr(), 64);
    DeviceMatrix Pr = R.permute(rperm32.ptr(), nullptr);
    out.csr("permute", Pm); out.csr("permute_cols64", Pc); out.csr("permute_rows", Pr);
    const DeviceMatrix *g1[4] = {&R, &B, &Bt, nullptr};
    const DeviceMatrix *g2[4] = {&R, &R, nullptr, &R};
    const DeviceMatrix *g3[4] = {&R, &B, nullptr, nullptr};
    const int row_sizes[2] = {R.rows(), 40};
    DeviceMatrix K1 = DeviceMatrix::bmat(2, 2, g1), K2 = DeviceMatrix::bmat(2, 2, g2), K3 = DeviceMatrix::bmat(2, 2, g3, row_sizes);
    out.csr("bmat", K1); out.csr("bmat_same_block", K2); out.csr("bmat_null_row", K3);
    {  // scale works in place: on uploads of their own
      DeviceMatrix X(hR), Y(hB);
      Vector dl = face::load_vec(in + "dl.f64"), dr = face::load_vec(in + "dr.f64"), dlB = face::load_vec(in + "dlB.f64"), drB = face::load_vec(in + "drB.f64");
      X.scale(&dl, nullptr); out.csr("scale_left", X);
      X.scale(nullptr, &dr); out.csr("scale_right", X);
      Y.scale(&dlB, &drB); out.csr("scale_both", Y);
      dlB[1] = 3.0;                                                      // a pending element write reaches the device before the call
      Y.scale(&dlB, nullptr); out.csr("scale_after_write", Y);
    }
    {  // gather and scatter
      Vector x = face::load_vec(in + "x.f64"), y(gidx32.n), y64(gidx64.n), back(x.size()), back64(x.size());
      int64_t bad = -7;
      x.gather(gidx32.ptr(), gidx32.n, 32, y);
      out.vec("gather", y);
      x.gather(gidx64.ptr(), gidx64.n, 64, y64, &bad);
      out.vec("gather64", y64); out.count("gather64_bad", bad);
      bad = -7;
      y.scatter(gidx32.ptr(), gidx32.n, 32, back, &bad);
      out.vec("scatter", back); out.count("scatter_bad", bad);
      y64.scatter(gidx64.ptr(), gidx64.n, 64, back64);
      out.vec("scatter64", back64);
      out.vec("spmv", Bt * x);                                           // rows() of a transposed rectangular matrix sizes the result
    }

    // ---- the same matrices from other values on the same patterns
    R.update_values(hR2); B.update_values(hB2);
    C.multiplyUpdate(R, B);
    out.csr("multiply_update", C);
    C.multiplyUpdate(R, B, &misses);
    out.csr("multiply_update_checked", C); out.count("multiply_misses", misses);
    misses = -7;
    Bt.transposeUpdate(B); Rt.transposeUpdate(R, &misses);
    out.csr("transpose_update", Bt); out.csr("transpose_update_checked", Rt); out.count("transpose_misses", misses);
    misses = -7;
    S.addUpdate(R, Rt, 1.5, -3.25, &misses);
    out.csr("add_update", S); out.count("add_misses", misses);
    S.addUpdate(R, Rt);
    out.csr("add_update_default", S);
    Eb.extractUpdate(R); out.csr("extract_update", Eb);
    Pm.permuteUpdate(R); out.csr("permute_update", Pm);
    K1.bmatUpdate(2, 2, g1); out.csr("bmat_update", K1);
  });
}
