"""numpy model of mgs_minres_plan (include/mgs.h, multigridsolver_amd/csrc/minres_plan.hip): the state block, the scalar steps, the
`frozen` / `apply` flags, the two predicated vector passes, the cycles and SpMVs that frozen iterations still run on the two alternating
(v, z̃) pairs, and the two host sides — the loop of mgs_minres_plan_solve with `ahead` (krylov_lookahead.hpp's rule), and
mgs_minres_plan_enqueue + FINAL.  tests/test_minres_plan_ref_cpu.py shows it equal to tests/minres_ref.py (status, iterations, reported
residual, every bit of x) for every `ahead`; the device code is held to mgs_minres in tests/test_gpu_minres_plan.py.

The "device" of the model runs every launch the moment it is enqueued — one of the schedules a stream allows, and the result must not
depend on which.  What a fold leaves for the next scalar step is modelled by `red`; inner products and norms use minres_ref's own helpers
(a norm is left as a norm: minres_ref takes √ of its own dot where the device takes √ of a folded one), so that equal statements give equal
bits.  `A` is an oracle_py.Csr or a callable v -> A·v, `precond` a callable v -> M·v or None."""
import numpy as np

from minres_ref import _dot, _norm, update_ref

RING = 1024      # posted slots; `ahead` is clamped to RING − 2 (krylov_lookahead.hpp)
WHY_EST, WHY_GAMMA = 1, 2


class State:
    """the state block"""
    def __init__(self):
        self.normb = self.gam = self.gam_prev = self.eta = self.kappa = self.delta = self.s0 = self.s1 = self.c0 = self.c1 = 0.0
        self.la = self.lb = self.lc = self.inv_g = self.a3 = self.a2 = self.a1 = self.step = self.resid = self.true_resid = 0.0
        self.it = 0; self.status = -1; self.frozen = 0; self.why = 0; self.wasted = 0; self.apply = 0


class MinresPlanModel:
    def __init__(self, A, precond=None):
        self.spmv = A if callable(A) else A.spmv
        self.M = (lambda u: np.array(u, copy=True)) if precond is None else precond
        self.st = State()
        self.red = 0.0
        self.posts = {}        # ticket -> (it, status, frozen, why, resid, normb): the ring (no slot is rewritten before it has been read)
        self.seq = 0
        self.info = [0, 0, 0, 0, 0, 0]
        self.v = None
        self.checks = []       # (iteration, estimate, true residual) of every true-residual look of solve()

    # ---------------------------------------------------------------- device: scalar steps
    def _post(self):
        self.seq += 1
        s = self.st
        self.posts[self.seq] = (s.it, s.status, s.frozen, s.why, s.resid, s.normb)

    def step_normb(self):
        s = self.st
        s.__init__()
        s.normb = self.red if self.red != 0.0 else 1.0

    def step_init_res(self, tol):
        s = self.st
        s.resid = s.true_resid = self.red / s.normb
        if s.resid <= tol:
            s.frozen, s.status = 1, 0

    def step_init(self, post):
        s = self.st
        if not s.frozen:
            g2 = self.red
            if not g2 > 0:
                s.frozen, s.status = 1, 2
            else:
                s.gam = np.sqrt(g2); s.gam_prev = 1.0; s.eta = s.gam
                s.kappa = s.resid * s.normb / s.gam
                s.s0 = s.s1 = 0.0; s.c0 = s.c1 = 1.0
        if post:
            self._post()

    def step_lanczos(self, it):
        s = self.st
        s.apply = 0
        if s.frozen:
            s.wasted += 1
            return
        s.it = it
        s.delta = self.red / (s.gam * s.gam)
        s.la, s.lb, s.lc = 1 / s.gam, -(s.delta / s.gam), -(s.gam / s.gam_prev)

    def step_rotate(self, tol, post):
        s = self.st
        if not s.frozen:
            gn2 = self.red
            gam, delta, eta, s0, s1, c0, c1 = s.gam, s.delta, s.eta, s.s0, s.s1, s.c0, s.c1
            if not gn2 >= 0:
                s.frozen, s.status = 1, 2
            else:
                gamn = np.sqrt(gn2)
                a0 = c1 * delta - c0 * s1 * gam
                a1 = np.sqrt(a0 * a0 + gn2)
                a2 = s1 * delta + c0 * c1 * gam
                a3 = s0 * gam
                if a1 == 0:
                    s.frozen, s.status = 1, 3
                else:
                    cn = a0 / a1; sn = gamn / a1
                    s.inv_g, s.a3, s.a2, s.a1, s.step, s.apply = 1 / gam, a3, a2, a1, cn * eta, 1
                    s.eta = -sn * eta
                    s.s0, s.s1, s.c0, s.c1, s.gam_prev, s.gam = s1, sn, c1, cn, gam, gamn
                    s.resid = s.kappa * abs(s.eta) / s.normb
                    why = (WHY_EST if s.resid < tol else 0) | (WHY_GAMMA if gamn == 0 else 0)
                    if why:
                        s.frozen, s.status, s.why = 1, 0, why
        if post:
            self._post()

    def step_recal(self, resid):
        s = self.st
        s.kappa = resid * s.normb / abs(s.eta)
        s.resid = s.true_resid = resid
        s.frozen, s.status, s.why, s.apply = 0, -1, 0, 0

    def step_final(self, iters, tol):
        s = self.st
        s.true_resid = self.red / s.normb
        s.apply = 0
        if not s.frozen:
            s.it, s.status = iters, 1
        elif s.status == 0:
            ok = s.true_resid <= tol if s.it == 0 else s.true_resid < tol
            s.status = 0 if ok else (3 if s.why & WHY_GAMMA else 1)
        s.frozen = 1

    # ---------------------------------------------------------------- device: vector passes (predicated on the state)
    def pass_lanczos(self, q, v, k_prev):
        """v_new = la·q + lb·v + lc·v_prev over v_prev = self.v[k_prev]; the c == 0.0 form does not read v_prev"""
        s = self.st
        if s.frozen:
            return
        if s.lc == 0.0:
            self.v[k_prev] = s.la * q + s.lb * v
        else:
            self.v[k_prev] = s.la * q + s.lb * v + s.lc * self.v[k_prev]

    def pass_update(self, z, k_prev, w):
        s = self.st
        if not s.apply:
            return
        self.w[k_prev], self.x = update_ref(s.inv_g, s.a3, s.a2, s.a1, s.step, z, self.w[k_prev], w, self.x)

    def true_residual(self):
        r = self.b - self.spmv(self.x)
        self.red = _norm(r)
        return r

    # ---------------------------------------------------------------- the launch sequences
    def enqueue_init(self, tol, post):
        self.red = _norm(self.b)
        self.step_normb()
        self.v[0] = self.true_residual()
        self.step_init_res(tol)
        self.zt[0] = self.M(self.v[0])
        self.red = _dot(self.zt[0], self.v[0])
        self.step_init(post)
        self.v[1] = np.zeros_like(self.b); self.w[0] = np.zeros_like(self.b); self.w[1] = np.zeros_like(self.b)

    def enqueue_iteration(self, it, tol, post):
        """SpMV with q·z̃ · LANCZOS · Lanczos pass · cycle · dot · ROTATE · update pass; the roles by the parity of `it`.  A frozen iteration
        runs SpMV, cycle and the reductions all the same: its cycle rewrites z̃[1 − cur] from the unchanged v[1 − cur]"""
        cur = (it - 1) & 1; wc = 1 - cur
        self.q = self.spmv(self.zt[cur])
        self.red = _dot(self.q, self.zt[cur])
        self.step_lanczos(it)
        self.pass_lanczos(self.q, self.v[cur], 1 - cur)
        self.zt[1 - cur] = self.M(self.v[1 - cur])
        self.red = _dot(self.zt[1 - cur], self.v[1 - cur])
        self.info[2] += 1
        self.step_rotate(tol, post)
        self.pass_update(self.zt[cur], 1 - wc, self.w[wc])

    def _begin(self, b, x0):
        self.b = np.ascontiguousarray(b, dtype=np.float64)
        self.x = np.zeros(self.b.shape[0]) if x0 is None else np.array(x0, dtype=np.float64)
        self.info[1] += 1
        self.info[2:] = [0, 0, 0, 0]
        self.checks = []
        if self.v is None or self.v[0].shape != self.b.shape:      # the plan's vectors are zeroed once, at create
            self.v = [np.zeros_like(self.b) for _ in range(2)]
            self.zt = [np.zeros_like(self.b) for _ in range(2)]
            self.w = [np.zeros_like(self.b) for _ in range(2)]
            self.q = np.zeros_like(self.b)

    # ---------------------------------------------------------------- host: enqueue-only
    def enqueue(self, b, iters, tol, x0=None):
        """→ (status, iterations done, true residual, x); no host look at all"""
        self._begin(b, x0)
        self.enqueue_init(tol, False)
        for i in range(1, iters + 1):
            self.enqueue_iteration(i, tol, False)
        self.q = self.true_residual()
        self.step_final(iters, tol)
        s = self.st
        self.info[3] = s.wasted
        return s.status, s.it, s.true_resid, self.x

    # ---------------------------------------------------------------- host: the blocking solve
    def _wait(self, ticket):
        self.info[4] += 1
        return self.posts.pop(ticket)

    def solve(self, b, max_iter, tol, ahead, x0=None):
        """→ (status, iterations, resid, x): mgs_minres's contract"""
        assert ahead >= 0
        self._begin(b, x0)
        win = min(ahead, RING - 2)
        self.enqueue_init(tol, True)
        out = [(0, self.seq)]            # enqueued, outcome not seen yet
        nxt, seen = 1, -1
        resid, normb = None, 1.0
        while True:
            while nxt <= max_iter and nxt - 1 - win <= seen:
                self.enqueue_iteration(nxt, tol, True)
                out.append((nxt, self.seq))
                nxt += 1
            assert len(out) <= RING - 1
            if not out:
                break
            need = max(nxt - 1 - win, out[0][0]) if nxt <= max_iter else out[-1][0]
            while out[0][0] < need:
                out.pop(0)
            it, status, frozen, why, resid, normb = self._wait(out.pop(0)[1])
            seen = need
            if not frozen:
                continue
            if it == 0:
                return self._done(status, 0, resid)
            est = resid
            self.q = self.b - self.spmv(self.x)          # a synchronising look, as in mgs_minres
            resid = _norm(self.q) / normb
            if status in (2, 3):
                return self._done(status, it, resid)
            self.checks.append((it, float(est), float(resid)))
            if resid < tol:
                return self._done(0, it, resid)
            if why & WHY_GAMMA:
                return self._done(3, it, resid)
            if it == max_iter:
                return self._done(1, max_iter, resid)
            self.step_recal(resid)
            self.info[5] += 1
            nxt, seen, out = it + 1, it, []
        if max_iter <= 0:
            return self._done(1, 0, resid)
        self.q = self.b - self.spmv(self.x)
        return self._done(1, max_iter, _norm(self.q) / normb)

    def _done(self, status, it, resid):
        self.info[3] = self.st.wasted
        return status, it, resid, self.x
