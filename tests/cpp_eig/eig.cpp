// The block-vector wrappers and LOBPCGiml of mgs_host.hpp on the device (tests/test_gpu_cpp_eig.py runs the Python face on the same files).
// In: A.mtx (symmetric), x0.f64 … x3.f64 (start vectors), c.f64 (a 4 × 3 coefficient matrix, row-major).
#include "face_io.hpp"
using namespace mgs;

int main(int argc, char **argv) {
  return face::run(argc, argv, [](const std::string &in, face::Out &out) {
    DeviceMatrix A(readMatrix(in + "A.mtx"));
    std::vector<Vector> X0;
    for (int j = 0; j < 4; ++j) X0.push_back(face::load_vec(in + "x" + std::to_string(j) + ".f64"));
    const std::vector<double> C = face::read_raw<double>(in + "c.f64");

    out.f64("gram_same", vecsGram(X0, X0));
    std::vector<Vector> two(X0.begin(), X0.begin() + 2);
    out.f64("gram_4x2", vecsGram(X0, two));
    std::vector<Vector> Y;
    for (int j = 0; j < 3; ++j) Y.push_back(Vector(A.rows()));
    vecsCombine(X0, C, Y);
    for (int j = 0; j < 3; ++j) out.vec("combine" + std::to_string(j), Y[(size_t)j]);

    {  // no preconditioner
      std::vector<Vector> X(X0);
      std::vector<double> theta, resid;
      int max_iter = 200; double tol = 1e-6;
      const int st = LOBPCGiml(A, X, theta, resid, nullptr, max_iter, tol);
      out.count("none.status", st); out.count("none.iterations", max_iter); out.number("none.tol", tol);
      out.f64("none.theta", theta); out.f64("none.resid", resid);
      for (int j = 0; j < 4; ++j) out.vec("none.x" + std::to_string(j), X[(size_t)j]);
    }
    {  // the hierarchy, in CGiml's calling shape
      PrecondOptions o; o.omega = 0.5; o.coarse_rows = 30;
      MultiGridPrecond M(A, nullptr, o);
      std::vector<Vector> X(X0);
      std::vector<double> theta;
      int max_iter = 200; double tol = 1e-6;
      const int st = LOBPCGiml(A, X, theta, M, max_iter, tol);
      out.count("amg.levels", M.levels());
      out.count("amg.status", st); out.count("amg.iterations", max_iter); out.number("amg.tol", tol);
      out.f64("amg.theta", theta);
      for (int j = 0; j < 4; ++j) out.vec("amg.x" + std::to_string(j), X[(size_t)j]);
    }
  });
}
