"""FgcrPlanModel: a model of mgs_fgcr_plan (include/mgs.h, multigridsolver_amd/csrc/fgcr_plan.hip) in plain float64 numpy: the state block, the
scalar steps (NORMB, INIT, COEF, RHOK, RES, YSOLVE, WIN, RESUME, FINAL), the `frozen` / `why` / `m_open` flags, the predicated vector passes, and
the two host sides — the loop of mgs_fgcr_plan_solve with `ahead` (speculative iterations that run past a freeze and across a scheduled close,
the close the host enqueues behind a posted freeze, the restart from the true residual), and mgs_fgcr_plan_enqueue + result.

The "device" of the model runs every launch the moment it is enqueued — one of the schedules a stream allows, and the result must not depend on
which.  What a fold leaves for the next scalar step is modelled by `red`.  The model and tests/fgcr_ref.py take inner products with the same
helper and form the same expressions, so equal statements give equal bits."""
import numpy as np

from fgcr_ref import _dot, _spmv_of, maxpy, proj

RING = 1024      # posted slots; `ahead` is clamped to RING − 2 (fgcr_plan.hip)
FW = 16          # the widest window

WHY_NONE, WHY_RECURSION, WHY_BREAKDOWN, WHY_INIT, WHY_TRUE = 0, 1, 2, 3, 4
ST_RUNNING, ST_OK, ST_BREAKDOWN, ST_RECURSION, ST_DRIFTED = -1, 0, 2, 4, 5


class State:
    """the state block; ρ, α, h, y, cf and U keep their values across solves, as device memory does"""
    def __init__(self):
        z = np.float64(0.0)
        self.rho = [z] * FW; self.alpha = [z] * FW; self.hj = [z] * FW; self.y = [z] * FW; self.cf = [z] * FW
        self.U = [[z] * FW for _ in range(FW)]
        self.fresh()

    def fresh(self):
        self.normb = self.resid = self.true_resid = self.rr = np.float64(0.0)
        self.it = 0; self.status = ST_RUNNING; self.frozen = 0; self.why = WHY_NONE; self.m_open = 0; self.wasted = 0


class FgcrPlanModel:
    def __init__(self, A, precond=None, restart=10, project=False):
        assert 1 <= restart <= FW
        self.spmv = _spmv_of(A)
        self.M = (lambda v: np.array(v, copy=True)) if precond is None else precond
        self.R = restart
        self.ns = project
        self.st = State()
        self.red = [0.0, 0.0]
        self.posts = {}        # ticket -> (it, status, frozen, why, resid): the ring (no slot is rewritten before it has been read)
        self.seq = 0
        self.info = [0, 0, 0, 0, 0, 0]
        self.r = None
        self.x_passes = 0      # x-passes that found an open window

    # ---------------------------------------------------------------- device: scalar steps
    def _post(self):
        self.seq += 1
        s = self.st
        self.posts[self.seq] = (s.it, s.status, s.frozen, s.why, s.resid)

    def step_normb(self):
        s = self.st
        s.fresh()
        nb = np.sqrt(self.red[0])
        s.normb = nb if nb != 0.0 else np.float64(1.0)

    def step_init(self, tol, post):
        s = self.st
        s.rr = self.red[0]
        s.resid = np.sqrt(s.rr) / s.normb
        if s.resid <= tol:
            s.frozen, s.status, s.why = 1, ST_OK, WHY_INIT
        if post:
            self._post()

    def step_coef(self, k):
        s = self.st
        if s.frozen:
            return
        for j in range(k):
            s.U[j][k] = s.hj[j] / s.rho[j] if s.rho[j] != 0.0 else np.float64(0.0)

    def step_rhok(self, k, it):
        s = self.st
        if s.frozen:
            s.wasted += 1
            return
        s.it = it
        s.rho[k] = self.red[0]
        s.m_open = k + 1
        if s.rho[k] == 0.0:
            s.alpha[k] = np.float64(0.0)
            s.frozen, s.status, s.why = 1, ST_BREAKDOWN, WHY_BREAKDOWN
            return
        s.alpha[k] = self.red[1] / s.rho[k]

    def step_res(self, tol, post):
        s = self.st
        if not s.frozen:
            s.rr = self.red[0]
            s.resid = np.sqrt(s.rr) / s.normb
            if s.resid < tol:
                s.frozen, s.status, s.why = 1, ST_RECURSION, WHY_RECURSION
        if post:
            self._post()

    def step_ysolve(self):
        s = self.st
        m = s.m_open
        for q in range(m - 1, -1, -1):
            t = s.alpha[q]
            for p in range(q + 1, m):
                t = t - s.U[q][p] * s.y[p]
            s.y[q] = t
        for q in range(m):
            s.cf[q] = -s.y[q]

    def step_win(self, tol, post):
        s = self.st
        t = np.sqrt(self.red[0]) / s.normb
        s.true_resid = t
        if not s.frozen:
            s.resid = t
            if t < tol:
                s.frozen, s.status, s.why = 1, ST_OK, WHY_TRUE
        elif s.why == WHY_RECURSION:
            s.resid = t; s.status = ST_OK if t < tol else ST_DRIFTED
        elif s.why == WHY_BREAKDOWN:
            s.resid = t; s.status = ST_OK if t < tol else ST_BREAKDOWN
        s.m_open = 0
        if post:
            self._post()

    def step_resume(self):
        s = self.st
        s.frozen, s.status, s.why, s.m_open = 0, ST_RUNNING, WHY_NONE, 0

    def step_final(self, iters, tol):
        s = self.st
        t = np.sqrt(self.red[0]) / s.normb
        s.true_resid = t
        if not s.frozen:
            s.it = iters; s.status = 0 if t < tol else 1
        elif s.why == WHY_INIT:
            s.status = 0 if t <= tol else 1
        elif s.why == WHY_BREAKDOWN:
            s.status = 0 if t < tol else 2
        else:
            s.status = 0 if t < tol else 1
        s.frozen = 1; s.m_open = 0

    # ---------------------------------------------------------------- device: vector passes (predicated on the state)
    def pass_orth(self, k):
        s = self.st
        if s.frozen:
            return                      # V[k] and the partials stay; RHOK ignores the fold
        self.V[k] = maxpy(self.V[k], self.V[:k], [s.U[j][k] for j in range(k)])
        self.red = [_dot(self.V[k], self.V[k]), _dot(self.V[k], self.r)]

    def pass_resid(self, k):
        s = self.st
        if s.frozen:
            return
        self.r = 1.0 * self.r + (-s.alpha[k]) * self.V[k]
        self.red = [_dot(self.r, self.r), 0.0]

    def pass_x(self):
        s = self.st
        m = s.m_open
        if m <= 0:
            return
        self.x_passes += 1
        self.x = maxpy(self.x, self.C[:m], [s.cf[q] for q in range(m)])

    # ---------------------------------------------------------------- the launch sequences
    def true_residual(self):
        self.r = self.b - self.spmv(self.x)
        if self.ns:
            self.r = proj(self.r)
        self.red = [_dot(self.r, self.r), 0.0]

    def enqueue_init(self, tol, post):
        pb = proj(self.b) if self.ns else self.b
        self.red = [_dot(pb, pb), 0.0]
        self.step_normb()
        if self.ns:
            self.x = proj(self.x)
        self.true_residual()
        self.step_init(tol, post)

    def enqueue_iteration(self, k, it, tol, post):
        """cycle · SpMV · dots · COEF · orth · RHOK · r-pass · RES; a frozen iteration runs cycle, SpMV and the reductions all the same, and the
        model asserts that they write slots behind the open ones only"""
        assert not (self.st.frozen and k < self.st.m_open), "a frozen iteration overwrites a direction of the open window"
        self.C[k] = self.M(self.r)
        if self.ns:
            self.C[k] = proj(self.C[k])
        self.V[k] = self.spmv(self.C[k])
        if k == 0:
            self.red = [_dot(self.V[0], self.V[0]), _dot(self.V[0], self.r)]
        else:
            for j in range(k):
                self.st.hj[j] = _dot(self.V[k], self.V[j])
            self.step_coef(k)
            self.pass_orth(k)
        self.step_rhok(k, it)
        self.pass_resid(k)
        self.info[2] += 1
        self.step_res(tol, post)

    def enqueue_close(self, project, it, tol, post, last):
        self.step_ysolve()
        self.pass_x()
        if project and self.ns:
            self.x = proj(self.x)
        self.true_residual()
        if last:
            self.step_final(it, tol)
        else:
            self.step_win(tol, post)

    def _begin(self, b, x0):
        self.b = np.ascontiguousarray(b, dtype=np.float64)
        self.x = np.zeros(self.b.shape[0]) if x0 is None else np.array(x0, dtype=np.float64)
        self.info[1] += 1
        self.info[2:] = [0, 0, 0, 0]
        if self.r is None or self.r.shape != self.b.shape:      # the plan's vectors are zeroed once, at create
            self.r = np.zeros_like(self.b)
            self.C = [np.zeros_like(self.b) for _ in range(self.R)]
            self.V = [np.zeros_like(self.b) for _ in range(self.R)]

    # ---------------------------------------------------------------- host: enqueue-only
    def enqueue(self, b, iters, tol, x0=None):
        """→ (status, iterations done, true residual, recursive residual, x); no host look at all"""
        with np.errstate(all="ignore"):
            self._begin(b, x0)
            self.enqueue_init(tol, False)
            k = 0
            for i in range(1, iters + 1):
                self.enqueue_iteration(k, i, tol, False)
                k += 1
                if k == self.R and i < iters:
                    self.enqueue_close(False, i, tol, False, False)
                    k = 0
            self.enqueue_close(iters > 0, iters, tol, False, True)
        s = self.st
        self.info[3] = s.wasted
        return s.status, s.it, s.true_resid, s.resid, self.x

    # ---------------------------------------------------------------- host: the blocking solve
    def _wait(self, ticket):
        self.info[4] += 1
        return self.posts.pop(ticket)

    def solve(self, b, max_iter, tol, ahead, x0=None):
        """→ (status, iterations, resid, x): mgs_fgcr's contract (iterations = *max_iter on return)"""
        assert ahead >= 0
        with np.errstate(all="ignore"):
            self._begin(b, x0)
            self.posts.clear()
            win = min(ahead, RING - 2)
            R = self.R
            r_it, r_status = 0, 1
            self.enqueue_init(tol, True)
            r_resid = 0.0
            out = [(0, self.seq)]            # enqueued, outcome not seen yet
            nxt, k, seen = 1, 0, -1
            while True:
                while nxt <= max_iter and nxt - 1 - win <= seen:
                    closing = k == R - 1 and nxt < max_iter
                    self.enqueue_iteration(k, nxt, tol, not closing)
                    if closing:
                        self.enqueue_close(False, nxt, tol, True, False)
                    out.append((nxt, self.seq))
                    nxt += 1
                    k = 0 if closing else k + 1
                assert len(out) <= RING - 1
                need = max(nxt - 1 - win, out[0][0]) if nxt <= max_iter else out[-1][0]
                while out[0][0] < need:
                    out.pop(0)
                it, status, frozen, why, resid = self._wait(out.pop(0)[1])
                seen = need
                if not frozen:
                    if seen < max_iter:
                        continue
                    if seen == 0:
                        r_it, r_resid, r_status = 0, resid, 1
                        break
                    self.enqueue_close(True, max_iter, tol, True, False)
                    it, status, frozen, why, resid = self._wait(self.seq)
                    r_it, r_resid, r_status = max_iter, resid, (0 if frozen and status == ST_OK else 1)
                    break
                out = []
                r_it = it
                if why == WHY_INIT:
                    r_resid, r_status = resid, 0
                    break
                if why == WHY_TRUE:
                    if self.ns:
                        self.x = proj(self.x)
                    r_resid, r_status = resid, 0
                    break
                was = why
                self.enqueue_close(True, it, tol, True, False)
                it, status, frozen, why, resid = self._wait(self.seq)
                r_resid = resid
                if was == WHY_BREAKDOWN:
                    r_status = 0 if status == ST_OK else 2
                    break
                if status == ST_OK:
                    r_status = 0
                    break
                self.info[5] += 1
                r_status = 1
                if r_it >= max_iter:
                    break
                self.step_resume()
                nxt, seen, k = r_it + 1, r_it, 0
        self.info[3] = self.st.wasted
        return r_status, r_it, r_resid, self.x
