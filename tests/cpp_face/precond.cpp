// mgs::MultiGridPrecond: solve(v) under every option.  In: A2d.mtx + v2d.f64, A3d.mtx + v3d.f64, A10k.mtx + P10k.mtx + v10k.f64 (an operator with a
// prolongation file), N.mtx + bN.f64 (a pure-Neumann operator and a right-hand side of zero mean).
#include "face_io.hpp"
using namespace mgs;

static MultiGridPrecond::Options options(int nu1, int nu2) {
  MultiGridPrecond::Options o;
  o.omega = 0.6; o.nu1 = nu1; o.nu2 = nu2; o.coarse_rows = 50;
  return o;
}
static void cycle(face::Out &out, const std::string &name, const MultiGridPrecond &M, const Vector &v) {
  out.vec(name, M.solve(v));
  out.count(name + ".levels", M.levels());
  out.count(name + ".precision0", M.operand_precision(0));
  out.count(name + ".symmetric", M.symmetric());
}

int main(int argc, char **argv) {
  return face::run(argc, argv, [](const std::string &in, face::Out &out) {
    const SMatrix A2 = readMatrix(in + "A2d.mtx"), A3 = readMatrix(in + "A3d.mtx");
    const Vector v2 = face::load_vec(in + "v2d.f64"), v3 = face::load_vec(in + "v3d.f64");
    DeviceMatrix A2d(A2), A3d(A3);
    cycle(out, "v11", MultiGridPrecond(A2d, nullptr, options(1, 1)), v2);
    cycle(out, "v21", MultiGridPrecond(A2d, nullptr, options(2, 1)), v2);
    cycle(out, "v02", MultiGridPrecond(A2d, nullptr, options(0, 2)), v2);
    cycle(out, "v11_3d", MultiGridPrecond(A3d, nullptr, options(1, 1)), v3);
    { MultiGridPrecond::Options o = options(1, 1); o.correction_scale = 1.6; cycle(out, "sigma", MultiGridPrecond(A2d, nullptr, o), v2); }
    { MultiGridPrecond::Options o = options(1, 1); o.multiplicative_precond = false; cycle(out, "additive", MultiGridPrecond(A2d, nullptr, o), v2); }
    {
      MultiGridPrecond::Options o = options(1, 1); o.use_preconditioner = false;
      MultiGridPrecond M(A2d, nullptr, o);
      out.vec("identity", M.solve(v2)); out.count("identity.use", M.use_preconditioner());
    }
    {
      MultiGridPrecond M(A2d, nullptr, options(1, 1));
      M.set_operand_precision(32);
      cycle(out, "fp32", M, v2);
      M.set_operand_precision(64);
      cycle(out, "fp64_again", M, v2);
    }
    {  // with a prolongation file, through both constructors; without it
      const SMatrix A = readMatrix(in + "A10k.mtx"), P = readMatrix(in + "P10k.mtx");
      const Vector v = face::load_vec(in + "v10k.f64");
      cycle(out, "with_P", MultiGridPrecond(A, P, options(1, 1)), v);
      DeviceMatrix Ad(A);
      cycle(out, "with_P_device", MultiGridPrecond(Ad, &P, options(1, 1)), v);
      cycle(out, "without_P", MultiGridPrecond(Ad, nullptr, options(1, 1)), v);
    }
    {  // a declared constant null space, then CGiml
      const SMatrix N = readMatrix(in + "N.mtx");
      DeviceMatrix Nd(N);
      out.count("nullspace.before", Nd.nullspaceConstant());
      Nd.setNullspaceConstant(true);
      out.count("nullspace.after", Nd.nullspaceConstant());
      MultiGridPrecond M(Nd, nullptr, options(1, 1));
      const Vector b = face::load_vec(in + "bN.f64");
      cycle(out, "nullspace.cycle", M, b);
      Vector x(N.rows()); x.setZero();
      int it = 200; double tol = 1e-8;
      out.count("nullspace.status", CGiml(Nd, x, b, M, it, tol));
      out.count("nullspace.iterations", it); out.number("nullspace.tol", tol);
      out.vec("nullspace.x", x);
      Nd.setNullspaceConstant(false);
      out.count("nullspace.withdrawn", Nd.nullspaceConstant());
    }
  });
}
