// Stand-alone driver of multigridsolver_amd/csrc/eig_dense.hpp (tests/test_eig_dense_cpu.py): host code only, no device, no libmgs.
// `program IN OUT`: IN holds doubles [mode, n, m_rule, G_A (n·n), G_B (n·n, mode 1 only)], row-major.  mode 0: jacobi(G_A); mode 1:
// generalized(G_A, G_B).  OUT receives doubles [return value, theta (n), V (n·n)].
#include <cstdio>
#include <vector>

#include "eig_dense.hpp"

int main(int argc, char **argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 1; }
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  double head[3];
  if (std::fread(head, sizeof(double), 3, f) != 3) { std::fclose(f); return 2; }
  const int mode = (int)head[0], n = (int)head[1], m_rule = (int)head[2];
  if (n < 1 || n > 64 || mode < 0 || mode > 1) { std::fclose(f); return 2; }
  const size_t nn = (size_t)n * n;
  std::vector<double> GA(nn), GB(nn), theta((size_t)n), V(nn);
  bool ok = std::fread(GA.data(), sizeof(double), nn, f) == nn;
  if (ok && mode == 1) ok = std::fread(GB.data(), sizeof(double), nn, f) == nn;
  std::fclose(f);
  if (!ok) return 2;
  const double ret = mode == 0 ? (double)eig_dense::jacobi(n, GA.data(), theta.data(), V.data())
                               : (double)eig_dense::generalized(n, GA.data(), GB.data(), m_rule, theta.data(), V.data());
  FILE *g = std::fopen(argv[2], "wb");
  if (!g) return 2;
  std::fwrite(&ret, sizeof(double), 1, g);
  std::fwrite(theta.data(), sizeof(double), (size_t)n, g);
  std::fwrite(V.data(), sizeof(double), nn, g);
  std::fclose(g);
  return 0;
}
