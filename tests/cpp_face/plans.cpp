// The four Krylov plans and SolutionGuess.  In: A2d.mtx, A2d_new.mtx (its pattern, other values), b0.f64, b1.f64, b2.f64; K.mtx + Bd.mtx + Pd.mtx +
// bK.f64 (the saddle-point system of solvers.cpp).  Every plan is built from a DeviceMatrix and a MultiGridPrecond that are gone before its first solve.
#include "face_io.hpp"
using namespace mgs;

static MultiGridPrecond::Options options() {
  MultiGridPrecond::Options o; o.omega = 0.6; o.coarse_rows = 50;
  return o;
}
template <class Plan> static Plan on_poisson(const std::string &in) {
  DeviceMatrix Ad(readMatrix(in + "A2d.mtx"));
  MultiGridPrecond M(Ad, nullptr, options());
  return Plan(Ad, M);
}
static FgcrPlan fgcr_on_poisson(const std::string &in) {
  DeviceMatrix Ad(readMatrix(in + "A2d.mtx"));
  MultiGridPrecond M(Ad, nullptr, options());
  return FgcrPlan(Ad, M, 4);
}
static MinresPlan minres_on_saddle(const std::string &in) {
  DeviceMatrix Kd(readMatrix(in + "K.mtx"));
  MultiGridPrecond::Options o; o.omega = 0.6;
  MultiGridPrecond M(readMatrix(in + "Bd.mtx"), readMatrix(in + "Pd.mtx"), o);
  return MinresPlan(Kd, M);
}
static SolutionGuess guess_on_poisson(const std::string &in) {
  DeviceMatrix Ad(readMatrix(in + "A2d.mtx"));
  return SolutionGuess(Ad, MGS_GUESS_RESIDUAL, 3);
}

template <class Plan> static void walk(face::Out &out, const std::string &name, Plan &plan, const Vector &b, int enqueued) {
  const int64_t n = b.size();
  for (int ahead = 0; ahead <= 1; ++ahead) {
    const std::string tag = name + ".solve" + std::to_string(ahead);
    Vector x(n); x.setZero();
    int it = 300; double tol = 1e-8;
    out.count(tag + ".status", plan.solve(x, b, it, tol, ahead));
    out.count(tag + ".iterations", it); out.number(tag + ".tol", tol);
    out.vec(tag + ".x", x);
    for (int i = 0; i < 6; ++i) out.count(tag + ".info" + std::to_string(i), plan.info(i));
  }
  {
    Vector x(n); x.setZero();
    int it = -1; double resid = -1.0;
    plan.enqueue(x, b, enqueued, 1e-8);
    out.count(name + ".result.status", plan.result(it, resid));
    out.count(name + ".result.iterations", it); out.number(name + ".result.resid", resid);
    out.vec(name + ".result.x", x);
    for (int i = 0; i < 6; ++i) out.count(name + ".result.info" + std::to_string(i), plan.info(i));
  }
  {  // the default ahead
    Vector x(n); x.setZero();
    int it = 300; double tol = 1e-6;
    out.count(name + ".default.status", plan.solve(x, b, it, tol));
    out.count(name + ".default.iterations", it); out.number(name + ".default.tol", tol);
    out.count(name + ".default.info3", plan.info(3));
    out.vec(name + ".default.x", x);
  }
}

template <class Plan> static void recursive(face::Out &out, const std::string &name, Plan &plan, const Vector &b, int enqueued) {
  Vector x(b.size()); x.setZero();
  int it = -1; double resid = -1.0, rec = -1.0;
  plan.enqueue(x, b, enqueued, 1e-8);
  out.count(name + ".recursive.status", plan.result(it, resid, &rec));
  out.count(name + ".recursive.iterations", it); out.number(name + ".recursive.resid", resid); out.number(name + ".recursive.recursive_resid", rec);
}

int main(int argc, char **argv) {
  return face::run(argc, argv, [](const std::string &in, face::Out &out) {
    const Vector b0 = face::load_vec(in + "b0.f64"), b1 = face::load_vec(in + "b1.f64"), b2 = face::load_vec(in + "b2.f64"), bK = face::load_vec(in + "bK.f64");
    { PcgPlan p = on_poisson<PcgPlan>(in); walk(out, "pcg", p, b0, 6); }
    { BicgstabPlan p = on_poisson<BicgstabPlan>(in); walk(out, "bicgstab", p, b0, 4); recursive(out, "bicgstab", p, b1, 5); }
    { FgcrPlan p = fgcr_on_poisson(in); walk(out, "fgcr", p, b0, 6); recursive(out, "fgcr", p, b1, 7); }
    { MinresPlan p = minres_on_saddle(in); walk(out, "minres", p, bK, 10); recursive(out, "minres", p, bK, 12); }
    {  // a guess whose DeviceMatrix is gone
      SolutionGuess g = guess_on_poisson(in);
      Vector x(b0.size()); x.setZero();
      out.number("lifetime.apply_empty", g.apply(b0, x));
      out.count("lifetime.update", g.update(b1));                       // any vector spans a direction
      out.number("lifetime.apply", g.apply(b0, x));
      out.vec("lifetime.x0", x);
      out.count("lifetime.size", g.size()); out.count("lifetime.capacity", g.capacity());
    }
    {  // three right-hand sides, capacity 2: the third accepted solution restarts the basis
      const SMatrix A = readMatrix(in + "A2d.mtx"), A_new = readMatrix(in + "A2d_new.mtx");
      DeviceMatrix Ad(A);
      MultiGridPrecond M(Ad, nullptr, options());
      SolutionGuess g(Ad, MGS_GUESS_ENERGY, 2);
      const Vector *rhs[3] = {&b0, &b1, &b2};
      Vector x(A.rows());
      for (int k = 0; k < 3; ++k) {
        const std::string tag = "guess.step" + std::to_string(k);
        x.setZero();
        out.number(tag + ".apply", g.apply(*rhs[k], x));
        out.vec(tag + ".x0", x);
        int it = 300; double tol = 1e-8;
        out.count(tag + ".status", CGiml(Ad, x, *rhs[k], M, it, tol));
        out.count(tag + ".iterations", it);
        out.count(tag + ".added", g.update(x));
        out.count(tag + ".size", g.size()); out.count(tag + ".restarts", g.restarts()); out.count(tag + ".refused", g.refused());
      }
      out.count("guess.refused_again", g.update(x));                     // the solution just stored lies inside the span
      out.count("guess.refused", g.refused());
      Vector xa(A.rows());
      g.applyAsync(b0, xa);
      out.vec("guess.apply_async", xa);
      Ad.update_values(A_new);
      M.refresh();
      g.rebase();
      out.number("guess.rebased.apply", g.apply(b1, x));
      out.vec("guess.rebased.x0", x);
      out.count("guess.rebased.size", g.size()); out.count("guess.capacity", g.capacity());
      g.reset();
      out.count("guess.reset.size", g.size());
      out.number("guess.reset.apply", g.apply(b1, x));
      out.vec("guess.reset.x0", x);
    }
  });
}
