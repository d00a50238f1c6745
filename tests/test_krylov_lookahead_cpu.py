"""The look-ahead bookkeeping the three Krylov plans' solve() loops share (multigridsolver_amd/csrc/krylov_lookahead.hpp), without a device:
tests/krylov_lookahead_sim.cpp includes that header alone, is built here with a plain g++ and simulates a solve from its arguments; its
trace of events is held against the same rule restated below, and every trace against what the ring and info() rely on."""
import itertools
import os
import subprocess

import pytest

from conftest import REPO

RING = 1024      # posted slots; `ahead` is capped at RING − 2 (krylov_lookahead.hpp)


def trace_ref(maxit, ahead, freeze, restarts):
    """The rule in the words of the solve loops before they shared it: INIT is iteration 0 with the first ticket; iteration `nxt` may be
    enqueued while nxt <= maxit and nxt − 1 − win <= seen; the host then waits for iteration max(nxt − 1 − win, oldest outstanding) — with
    nothing left to enqueue, for the newest — and drops the older ones; a restart behind iteration i forgets what is outstanding and goes
    on with i + 1.  The device runs every step in stream order: behind a freeze an iteration runs frozen and posts the freeze."""
    win = min(ahead, RING - 2)
    drift = set(restarts)
    dev = {"it": 0, "frozen": 0, "wasted": 0}
    posts, events = {}, []

    def run(it, ticket):
        if dev["frozen"]:
            dev["wasted"] += it > 0
        else:
            dev["it"] = it
            dev["frozen"] = int(it == freeze or (it > 0 and it in drift))
        posts[ticket] = (dev["it"], dev["frozen"])
        events.append(("enqueue", it, ticket))

    seq = 1
    run(0, seq)
    out = [(0, seq)]
    nxt, seen = 1, -1
    while True:
        while nxt <= maxit and nxt - 1 - win <= seen:
            seq += 1
            run(nxt, seq)
            out.append((nxt, seq))
            nxt += 1
        if not out:
            break
        need = max(nxt - 1 - win, out[0][0]) if nxt <= maxit else out[-1][0]
        out = [o for o in out if o[0] >= need]
        (it, ticket), out = out[0], out[1:]
        assert it == need
        events.append(("wait", it, ticket))
        seen = need
        at, frozen = posts[ticket]
        if not frozen:
            continue
        if at == 0 or at == freeze or at not in drift or at >= maxit:
            break
        drift.discard(at)
        dev["frozen"] = 0
        events.append(("restart", at))
        out, nxt, seen = [], at + 1, at
    events.append(("end", dev["it"], dev["wasted"]))
    return events


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = tmp_path_factory.mktemp("lookahead") / "krylov_lookahead_sim"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(REPO, "multigridsolver_amd", "csrc"),
                        "-o", str(exe), os.path.join(REPO, "tests", "krylov_lookahead_sim.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(maxit, ahead, freeze, restarts):
        r = subprocess.run([str(exe), str(maxit), str(ahead), str(freeze)] + [str(i) for i in restarts], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        return [(w[0],) + tuple(int(v) for v in w[1:]) for w in (line.split() for line in r.stdout.splitlines())]
    return run


def cases():
    for maxit, ahead in itertools.product((0, 1, 2, 7), (0, 1, 3, 2000)):
        for freeze in sorted({-1, 0, 1, maxit}):
            for restarts in ((), (max(1, (maxit + 1) // 2),)):
                yield maxit, ahead, freeze, restarts
    yield RING + 76, 2000, -1, ()                      # more iterations than slots: the only case in which the cap of `ahead` binds


@pytest.mark.parametrize("maxit,ahead,freeze,restarts", list(cases()))
def test_trace(sim, maxit, ahead, freeze, restarts):
    events = sim(maxit, ahead, freeze, restarts)
    assert events == trace_ref(maxit, ahead, freeze, restarts)
    win = min(ahead, RING - 2)
    enqueued, passed, outstanding = {}, set(), []      # ticket → iteration; tickets waited for or skipped; tickets the host may still look at
    iterations, expect_next = 0, None
    for e in events[:-1]:
        if e[0] == "enqueue":
            _, it, ticket = e
            assert ticket not in enqueued and (not enqueued or ticket == max(enqueued) + 1)
            if expect_next is not None:                # after a restart at i, the next enqueue is i + 1
                assert it == expect_next
                expect_next = None
            enqueued[ticket] = it
            outstanding.append(ticket)
            iterations += it > 0
            assert len(outstanding) <= win + 1         # posts the ring must hold at this moment
        elif e[0] == "wait":
            _, it, ticket = e
            assert ticket in enqueued and enqueued[ticket] == it          # not waited for before it was enqueued
            assert ticket not in passed                                    # never again once skipped or waited for
            assert ticket in outstanding
            passed.update(t for t in outstanding if t <= ticket)
            outstanding = [t for t in outstanding if t > ticket]
        else:
            assert e[0] == "restart" and restarts and e[1] == restarts[0]
            passed.update(outstanding)                 # forgotten: never looked at
            outstanding = []
            expect_next = e[1] + 1
    assert expect_next is None
    _, it, wasted = events[-1]
    assert events[-1][0] == "end"
    assert iterations - it == wasted                   # info()[3]: the iterations that ran frozen
    restarted = any(e[0] == "restart" for e in events)
    if 0 <= freeze <= maxit and (not restarts or restarted or freeze <= restarts[0]):
        assert it == freeze
    if freeze < 0 and not restarts:
        assert it == maxit and wasted == 0 and iterations == maxit
