"""numpy model of mgs_pcg_plan (include/mgs.h, multigridsolver_amd/csrc/pcg_plan.hip): the state block, the five scalar steps, the
frozen / first / pending flags, the predicated vector passes, and the two host sides — the loop of mgs_pcg_plan_solve with `ahead`, and
mgs_pcg_plan_enqueue + result.  tests/test_pcg_plan_ref_cpu.py shows it equal to tests/pcg_ref.py (status, iterations, reported residual,
every bit of x) for every `ahead`; the device code is held to mgs_pcg in tests/test_gpu_pcg_plan.py.

The "device" of the model runs every launch the moment it is enqueued — one of the schedules a stream allows, and the result must not
depend on which.  What a fold leaves for the next scalar step is modelled by `red`; inner products and norms use pcg_ref's own helpers
(a norm is left as a norm: pcg_ref takes np.linalg.norm where the device takes √ of a folded r·r), so that equal statements give equal
bits.  `A` is an oracle_py.Csr or a callable v -> A·v, `precond` a callable v -> B·v or None."""
import numpy as np

from pcg_ref import _dot, _norm

RING = 1024      # posted slots; `ahead` is clamped to RING − 2 (pcg_plan.hip)


class State:
    """the state block"""
    def __init__(self):
        self.normb = self.rho = self.rho_prev = self.alpha = self.beta = self.pq = self.zq = self.rr = self.resid = self.true_resid = 0.0
        self.it = 0; self.status = -1; self.frozen = 0; self.first = 1; self.pending = 0; self.wasted = 0


class PcgPlanModel:
    def __init__(self, A, precond=None, flexible=False):
        self.spmv = A if callable(A) else A.spmv
        self.precond, self.flexible = precond, bool(flexible)
        self.st = State()
        self.red = [0.0, 0.0]
        self.posts = {}        # ticket -> (it, status, frozen, resid, normb): the ring (no slot is rewritten before it has been read)
        self.seq = 0
        self.info = [0, 0, 0, 0, 0, 0]
        self.r = self.z = self.p = self.q = None

    # ---------------------------------------------------------------- device: scalar steps
    def _post(self):
        self.seq += 1
        s = self.st
        self.posts[self.seq] = (s.it, s.status, s.frozen, s.resid, s.normb)

    def step_normb(self):
        s = self.st
        s.__init__()
        s.normb = self.red[0] if self.red[0] != 0.0 else 1.0

    def step_init(self, tol, post):
        s = self.st
        s.rr = self.red[0]
        s.resid = self.red[0] / s.normb
        if s.resid <= tol:
            s.frozen, s.status = 1, 0
        if post:
            self._post()

    def step_rho(self, it):
        s = self.st
        if s.frozen:
            s.wasted += 1
            return
        s.it = it
        s.rho, s.zq = self.red
        if not s.rho > 0:
            s.frozen, s.status = 1, 2
            return
        if not s.first:
            s.beta = -s.alpha * s.zq / s.rho_prev if self.flexible else s.rho / s.rho_prev

    def step_pq(self):
        s = self.st
        if s.frozen:
            return
        s.pq = self.red[0]
        s.first = s.pending = 0
        if not s.pq > 0:
            s.frozen, s.status = 1, 3
            return
        s.alpha = s.rho / s.pq
        s.pending = 1

    def step_res(self, tol, post):
        s = self.st
        if not s.frozen:
            s.rr = self.red[0]
            s.resid = self.red[0] / s.normb
            s.rho_prev = s.rho
            if s.resid < tol:
                s.frozen, s.status = 1, 0
        if post:
            self._post()

    def step_restart(self, resid):
        s = self.st
        s.frozen, s.status, s.first, s.pending, s.resid = 0, -1, 1, 0, resid

    def step_final(self, iters, tol):
        s = self.st
        s.true_resid = self.red[0] / s.normb
        s.pending = 0
        if not s.frozen:
            s.it, s.status = iters, 1
        elif s.status == 0:
            ok = s.true_resid <= tol if s.it == 0 else s.true_resid < tol
            s.status = 0 if ok else 1
        s.frozen = 1

    # ---------------------------------------------------------------- device: vector passes (predicated on the state)
    def pass_direction(self):
        s = self.st
        if s.frozen:
            return
        if s.first:
            self.p = self.z.copy()
        else:
            self.x = self.x + s.alpha * self.p
            self.p = self.z + s.beta * self.p

    def pass_residual(self):
        s = self.st
        if s.frozen:
            return                      # r and the partials stay; RES ignores the fold
        self.r = self.r - s.alpha * self.q
        self.red = [_norm(self.r), 0.0]

    def pass_flush(self):
        s = self.st
        if s.pending:
            self.x = self.x + s.alpha * self.p
        s.pending = 0                   # (its own one-wave step on the device)

    def true_residual(self):
        self.r = self.b - self.spmv(self.x)
        self.red = [_norm(self.r), 0.0]

    # ---------------------------------------------------------------- the launch sequences
    def enqueue_init(self, tol, post):
        self.red = [_norm(self.b), 0.0]
        self.step_normb()
        self.true_residual()
        self.step_init(tol, post)

    def enqueue_iteration(self, it, tol, first, post):
        """cycle (or copy) · dots + fold · RHO · direction · SpMV with p·q + fold · PQ · residual + fold · RES; frozen iterations run cycle,
        SpMV and the reductions all the same.  `first` is the host's copy of the flag: it chooses the one- or the two-product reduction."""
        self.z = np.array(self.r, copy=True) if self.precond is None else self.precond(self.r)
        self.red = [_dot(self.r, self.z), _dot(self.z, self.q) if (self.flexible and not first) else 0.0]
        self.step_rho(it)
        self.pass_direction()
        self.q = self.spmv(self.p)
        self.red = [_dot(self.p, self.q), 0.0]
        self.step_pq()
        self.pass_residual()
        self.info[2] += 1
        self.step_res(tol, post)

    def _begin(self, b, x0):
        self.b = np.ascontiguousarray(b, dtype=np.float64)
        self.x = np.zeros(self.b.shape[0]) if x0 is None else np.array(x0, dtype=np.float64)
        self.info[1] += 1
        self.info[2:] = [0, 0, 0, 0]
        if self.p is None or self.p.shape != self.b.shape:      # the plan's vectors are zeroed once, at create
            self.r, self.z, self.p, self.q = (np.zeros_like(self.b) for _ in range(4))

    # ---------------------------------------------------------------- host: enqueue-only
    def enqueue(self, b, iters, tol, x0=None):
        """→ (status, iterations done, true residual, x); no host look at all"""
        self._begin(b, x0)
        self.enqueue_init(tol, False)
        for i in range(1, iters + 1):
            self.enqueue_iteration(i, tol, i == 1, False)
        self.pass_flush()
        self.true_residual()
        self.step_final(iters, tol)
        s = self.st
        self.info[3] = s.wasted
        return s.status, s.it, s.true_resid, self.x

    # ---------------------------------------------------------------- host: the blocking solve
    def _wait(self, ticket):
        self.info[4] += 1
        return self.posts.pop(ticket)

    def solve(self, b, max_iter, tol, ahead, x0=None):
        """→ (status, iterations, resid, x): mgs_pcg's contract"""
        assert ahead >= 0
        self._begin(b, x0)
        win = min(ahead, RING - 2)
        self.enqueue_init(tol, True)
        out = [(0, self.seq)]            # enqueued, outcome not seen yet
        nxt, seen, first = 1, -1, True
        resid = None
        while True:
            while nxt <= max_iter and nxt - 1 - win <= seen:
                self.enqueue_iteration(nxt, tol, first, True)
                first = False
                out.append((nxt, self.seq))
                nxt += 1
            assert len(out) <= RING - 1
            if not out:
                break
            need = max(nxt - 1 - win, out[0][0]) if nxt <= max_iter else out[-1][0]
            while out[0][0] < need:
                out.pop(0)
            it, status, frozen, resid, normb = self._wait(out.pop(0)[1])
            seen = need
            if not frozen:
                continue
            if status in (2, 3):
                self.pass_flush()
                return self._done(status, it, resid)
            if it == 0:
                return self._done(0, 0, resid)
            self.pass_flush()
            self.r = self.b - self.spmv(self.x)          # the existing host path: a synchronising look
            resid = _norm(self.r) / normb
            if resid < tol:
                return self._done(0, it, resid)
            if it == max_iter:
                return self._done(1, max_iter, resid)
            self.step_restart(resid)
            self.info[5] += 1
            first, nxt, seen, out = True, it + 1, it, []
        self.pass_flush()
        return self._done(1, max_iter, resid)

    def _done(self, status, it, resid):
        self.info[3] = self.st.wasted
        return status, it, resid, self.x
