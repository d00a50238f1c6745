// CGiml, BiCGSTABiml and MINRESiml: the device-resident forms and the generic templates.  In: A2d.mtx + b2d.f64 (symmetric positive definite),
// K.mtx + Bd.mtx + Pd.mtx + bK.f64 (a saddle-point system, the block-diagonal operator its preconditioner is built on, and that operator's P).
#include "face_io.hpp"
using namespace mgs;

template <typename F> static void solve(face::Out &out, const std::string &name, int64_t n, F call) {
  Vector x(n); x.setZero();
  int it = 300; double tol = 1e-8;
  out.count(name + ".status", call(x, it, tol));
  out.count(name + ".iterations", it); out.number(name + ".tol", tol);
  out.vec(name + ".x", x);
}

int main(int argc, char **argv) {
  return face::run(argc, argv, [](const std::string &in, face::Out &out) {
    {
      const SMatrix A = readMatrix(in + "A2d.mtx");
      const Vector b = face::load_vec(in + "b2d.f64");
      DeviceMatrix Ad(A);
      MultiGridPrecond::Options o; o.omega = 0.6; o.coarse_rows = 50;
      MultiGridPrecond M(Ad, nullptr, o);
      solve(out, "cg", A.rows(), [&](Vector &x, int &it, double &tol) { return CGiml(Ad, x, b, M, it, tol); });
      solve(out, "cg_host_matrix", A.rows(), [&](Vector &x, int &it, double &tol) { return CGiml(A, x, b, M, it, tol); });
      solve(out, "bicgstab", A.rows(), [&](Vector &x, int &it, double &tol) { return BiCGSTABiml(Ad, x, b, M, it, tol); });
      solve(out, "cg_generic", A.rows(), [&](Vector &x, int &it, double &tol) { return CGiml<DeviceMatrix, Vector, MultiGridPrecond, double>(Ad, x, b, M, it, tol); });
      o.nu1 = 2;                                                         // not a fixed symmetric operator: the flexible form
      MultiGridPrecond M21(Ad, nullptr, o);
      solve(out, "cg_flexible", A.rows(), [&](Vector &x, int &it, double &tol) { return CGiml(Ad, x, b, M21, it, tol); });
    }
    {
      const SMatrix K = readMatrix(in + "K.mtx"), Bd = readMatrix(in + "Bd.mtx"), Pd = readMatrix(in + "Pd.mtx");
      const Vector b = face::load_vec(in + "bK.f64");
      DeviceMatrix Kd(K);
      MultiGridPrecond::Options o; o.omega = 0.6;
      MultiGridPrecond M(Bd, Pd, o);
      solve(out, "minres", K.rows(), [&](Vector &x, int &it, double &tol) { return MINRESiml(Kd, x, b, M, it, tol); });
      solve(out, "minres_host_matrix", Bd.rows(), [&](Vector &x, int &it, double &tol) { return MINRESiml(Bd, x, b, M, it, tol); });      // the preconditioner's own operator
      solve(out, "minres_generic", K.rows(), [&](Vector &x, int &it, double &tol) { return MINRESiml<DeviceMatrix, Vector, MultiGridPrecond, double>(Kd, x, b, M, it, tol); });
    }
  });
}
