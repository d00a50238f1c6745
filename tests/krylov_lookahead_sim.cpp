// krylov_lookahead_sim.cpp — the look-ahead bookkeeping of the Krylov plans' solve() (csrc/krylov_lookahead.hpp) driven without a device.
// usage: krylov_lookahead_sim MAXIT AHEAD FREEZE [RESTART ...]
//   FREEZE: the iteration at which the device freezes for good (0: INIT), −1: never
//   RESTART: iterations at which the recursion says converged and the true residual does not — the device freezes there once, and the host,
//   when it sees that freeze and the iteration is not the last, restarts behind it (pcg_plan.hip; fgcr_plan.hip's restart_now)
// The device is modelled as running every step at once, in stream order, which is all a post depends on: an iteration enqueued behind a
// freeze runs frozen (counted into `wasted`) and posts the freeze.  One line per event: `enqueue it ticket`, `wait it ticket`, `restart it`,
// and last `end it wasted` — the state's it and what info()[3] would report.  Built by tests/test_krylov_lookahead_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>

#include "krylov_lookahead.hpp"

int main(int argc, char **argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: %s MAXIT AHEAD FREEZE [RESTART ...]\n", argv[0]); return 2; }
  const int maxit = std::atoi(argv[1]), ahead = std::atoi(argv[2]), freeze = std::atoi(argv[3]);
  std::set<int> drift;
  for (int a = 4; a < argc; ++a) drift.insert(std::atoi(argv[a]));

  struct Post { int it, frozen; };
  std::map<unsigned long long, Post> ring;            // ticket → what the step posted
  int dev_it = 0, dev_frozen = 0, wasted = 0;
  unsigned long long seq = 0;
  auto run = [&](int it) {                            // the device's side of INIT (it = 0) or of one iteration, with its posting step
    if (dev_frozen) { if (it > 0) ++wasted; }
    else {
      dev_it = it;
      if (it == freeze || (it > 0 && drift.count(it))) dev_frozen = 1;
    }
    ring[++seq] = {dev_it, dev_frozen};
  };

  krylov::Lookahead la(maxit, ahead);
  run(0);
  std::printf("enqueue 0 %llu\n", seq);
  la.enqueued(seq);
  for (;;) {
    while (la.may_enqueue()) {
      run(la.next);
      std::printf("enqueue %d %llu\n", la.next, seq);
      la.enqueued(seq);
    }
    if (la.idle()) break;
    const unsigned long long ticket = la.take();
    std::printf("wait %d %llu\n", la.seen, ticket);
    if (!ring.count(ticket)) { std::printf("waited for a ticket that was never enqueued\n"); return 1; }
    const Post L = ring[ticket];
    if (!L.frozen) continue;
    if (L.it == 0 || L.it == freeze || !drift.count(L.it) || L.it >= maxit) break;
    drift.erase(L.it);                                // the solve goes on from the true residual behind iteration L.it
    dev_frozen = 0;
    std::printf("restart %d\n", L.it);
    la.restart(L.it);
  }
  std::printf("end %d %d\n", dev_it, wasted);
  return 0;
}
