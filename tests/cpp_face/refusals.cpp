// Refusals: every one is a validated error that reaches the caller as mgs::Error, and the context serves a correct operation afterwards.
// In: R.mtx, B.mtx (R.cols rows), Rq.mtx (R's shape, another pattern), x.f64, gbad.i32 (indices, some outside x), K.mtx + Bd.mtx + Pd.mtx.
#include "face_io.hpp"
using namespace mgs;

template <typename F> static void refused(face::Out &out, const std::string &name, F call) {
  long long code = 0;
  try { call(); }
  catch (const Error &e) { code = e.code; std::cout << name << ": " << e.what() << std::endl; }
  out.count(name + ".code", code);
}

int main(int argc, char **argv) {
  return face::run(argc, argv, [](const std::string &in, face::Out &out) {
    const SMatrix hR = readMatrix(in + "R.mtx"), hB = readMatrix(in + "B.mtx"), hRq = readMatrix(in + "Rq.mtx");
    DeviceMatrix R(hR), B(hB), Rq(hRq);
    const Vector x = face::load_vec(in + "x.f64");

    const DeviceMatrix *grid[4] = {&R, &B, nullptr, &R};
    DeviceMatrix K = DeviceMatrix::bmat(1, 2, grid);
    refused(out, "bmat_update_other_grid", [&] { K.bmatUpdate(2, 2, grid); });
    refused(out, "bmat_update_other_grid_1x1", [&] { K.bmatUpdate(1, 1, grid); });
    K.bmatUpdate(1, 2, grid);
    out.csr("after_bmat_update", K);

    DeviceMatrix C = R.multiply(B);
    int64_t misses = -7;
    refused(out, "multiply_update_other_pattern", [&] { C.multiplyUpdate(Rq, B, &misses); });
    out.count("multiply_update_other_pattern.misses", misses);
    misses = -7;
    C.multiplyUpdate(R, B, &misses);
    out.csr("after_multiply_update", C); out.count("after_multiply_update.misses", misses);

    face::DevList<int32_t> gbad(face::read_raw<int32_t>(in + "gbad.i32"));
    Vector y(gbad.n);
    int64_t bad = -7;
    refused(out, "gather_out_of_range", [&] { x.gather(gbad.ptr(), gbad.n, 32, y, &bad); });
    out.count("gather_out_of_range.bad", bad);
    out.vec("gather_out_of_range.y", y);                                // +0.0 where the index was refused
    out.vec("after_gather", R * x);

    refused(out, "update_values_other_pattern", [&] { R.update_values(hRq); });
    refused(out, "update_values_other_shape", [&] { R.update_values(hB); });
    out.csr("after_update_values", R);                                  // untouched

    {
      const SMatrix hK = readMatrix(in + "K.mtx");
      DeviceMatrix Kd(hK);
      MultiGridPrecond::Options o; o.omega = 0.6; o.nu1 = 2;
      MultiGridPrecond M21(readMatrix(in + "Bd.mtx"), readMatrix(in + "Pd.mtx"), o);
      refused(out, "minres_plan_v21", [&] { MinresPlan p(Kd, M21); });
      Vector xs(hK.rows()), bs(hK.rows());
      bs.upload(std::vector<double>((size_t)hK.rows(), 1.0));
      int it = 10; double tol = 1e-8;
      refused(out, "minres_v21", [&] { MINRESiml(Kd, xs, bs, M21, it, tol); });
      out.vec("after_minres", M21.solve(bs));
    }
  });
}
