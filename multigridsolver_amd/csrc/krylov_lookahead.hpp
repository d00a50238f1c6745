// krylov_lookahead.hpp — which posted outcome a plan's solve() looks at next (pcg_plan.hip, bicgstab_plan.hip, fgcr_plan.hip).
// Host code without a HIP include: tests/krylov_lookahead_sim.cpp builds it with a plain C++ compiler.
//
// A solve enqueues iterations and looks at their posted outcomes `ahead` iterations behind the queue.  INIT is iteration 0.  Every enqueue
// that posts is recorded with its ticket; the host then waits for the one outcome the next enqueue depends on and drops the older ones
// unread (a freeze is sticky: every later post shows it).
#pragma once
#include <algorithm>
#include <deque>

namespace krylov {
constexpr int RING = 1024;               // posted slots; at most RING − 1 posts are outstanding, so no slot is rewritten before the host has read it

struct Lookahead {
  struct Out { int it; unsigned long long ticket; };
  std::deque<Out> outq;                  // enqueued, outcome not seen yet
  int maxit, win;                        // at most win + 1 posts of iterations are outstanding
  int next = 0, seen = -1;               // next iteration to enqueue; outcomes are known through iteration `seen`

  Lookahead(int maxit_, int ahead) : maxit(maxit_), win(std::min(ahead, RING - 2)) {}
  bool may_enqueue() const { return next <= maxit && next - 1 - win <= seen; }
  void enqueued(unsigned long long ticket) { outq.push_back({next, ticket}); ++next; }
  bool idle() const { return outq.empty(); }          // every iteration up to maxit has been seen
  // the outcome the next enqueue waits for; with nothing left to enqueue, the last one.  Older ones are dropped.  → its ticket; `seen` moves on
  unsigned long long take() {
    const int need = next <= maxit ? std::max(next - 1 - win, outq.front().it) : outq.back().it;
    while (outq.front().it < need) outq.pop_front();
    const unsigned long long ticket = outq.front().ticket;
    outq.pop_front();
    seen = need;
    return ticket;
  }
  // the solve goes on from the true residual behind iteration i: what was enqueued past i ran frozen and is enqueued again
  void restart(int i) { outq.clear(); next = i + 1; seen = i; }
};
}   // namespace krylov
