// The generalised overload of LOBPCGiml and eigResidual of mgs_host.hpp on the device (tests/test_gpu_cpp_eig_gen.py runs the Python face on the
// same files).  In: A.mtx, B.mtx (symmetric, B positive definite), x0.f64 … x3.f64 (start vectors).
#include "face_io.hpp"
using namespace mgs;

int main(int argc, char **argv) {
  return face::run(argc, argv, [](const std::string &in, face::Out &out) {
    DeviceMatrix A(readMatrix(in + "A.mtx"));
    DeviceMatrix B(readMatrix(in + "B.mtx"));
    std::vector<Vector> X0;
    for (int j = 0; j < 4; ++j) X0.push_back(face::load_vec(in + "x" + std::to_string(j) + ".f64"));

    {  // the fused residual pass, out of place and in place
      Vector r(A.rows());
      out.number("res.nrm2", eigResidual(X0[0], X0[1], 0.625, r));
      out.vec("res.r", r);
      Vector a(X0[2]);
      out.number("res.inplace.nrm2", eigResidual(a, X0[3], -1.75, a));
      out.vec("res.inplace.r", a);
    }
    {  // no preconditioner
      std::vector<Vector> X(X0);
      std::vector<double> theta, resid;
      int max_iter = 200; double tol = 1e-6;
      const int st = LOBPCGiml(A, B, X, theta, resid, nullptr, max_iter, tol);
      out.count("none.status", st); out.count("none.iterations", max_iter); out.number("none.tol", tol);
      out.f64("none.theta", theta); out.f64("none.resid", resid);
      for (int j = 0; j < 4; ++j) out.vec("none.x" + std::to_string(j), X[(size_t)j]);
    }
    {  // the hierarchy
      PrecondOptions o; o.omega = 0.5; o.coarse_rows = 30;
      MultiGridPrecond M(A, nullptr, o);
      std::vector<Vector> X(X0);
      std::vector<double> theta, resid;
      int max_iter = 200; double tol = 1e-6;
      const int st = LOBPCGiml(A, B, X, theta, resid, &M, max_iter, tol);
      out.count("amg.levels", M.levels());
      out.count("amg.status", st); out.count("amg.iterations", max_iter); out.number("amg.tol", tol);
      out.f64("amg.theta", theta); out.f64("amg.resid", resid);
      for (int j = 0; j < 4; ++j) out.vec("amg.x" + std::to_string(j), X[(size_t)j]);
    }
  });
}
