"""Two things for the BiCGSTAB-plan tests, both plain float64 numpy:

bicgstab_ref   a restatement of mgs_bicgstab (multigridsolver_amd/csrc/krylov.hip; reference BiCGSTABiml, src/common/bicg.cpp:74-136) with the
               same statement order, the same `1.0*r + (−α)*v` forms and the same write-back.  → (status, iterations, resid, x), where
               `iterations` is what *max_iter holds on return (untouched on statuses 2 and 3).

BicgstabPlanModel   a model of mgs_bicgstab_plan (include/mgs.h, multigridsolver_amd/csrc/bicgstab_plan.hip): the state block, the scalar steps,
               the frozen / first / half flags, the predicated vector passes, and the two host sides — the loop of mgs_bicgstab_plan_solve
               with `ahead`, and mgs_bicgstab_plan_enqueue + result.

The "device" of the model runs every launch the moment it is enqueued — one of the schedules a stream allows, and the result must not
depend on which.  What a fold leaves for the next scalar step is modelled by `red`.  Both sides take inner products with the same helper
and form the same expressions, so equal statements give equal bits.  `A` is an oracle_py.Csr, a dense array or a callable v -> A·v;
`precond` a callable v -> M·v or None for the identity."""
import numpy as np

RING = 1024      # posted slots; `ahead` is clamped to RING − 2 (bicgstab_plan.hip)


def _dot(a, b):
    return np.float64(a @ b)      # a numpy scalar: x/0 gives ±inf or NaN as on the device, where a Python float would raise


def _spmv_of(A):
    if callable(A):
        return A
    if isinstance(A, np.ndarray):
        return lambda v: A @ v
    return A.spmv


def bicgstab_ref(A, b, precond=None, tol=1e-6, max_iter=10000, x0=None):
    spmv = _spmv_of(A)
    M = (lambda v: np.array(v, copy=True)) if precond is None else precond
    b = np.ascontiguousarray(b, dtype=np.float64)
    x = np.zeros(b.shape[0]) if x0 is None else np.array(x0, dtype=np.float64)
    with np.errstate(all="ignore"):
        normb = np.sqrt(_dot(b, b))                                   # :80
        r = b - spmv(x)                                               # :82
        rt = r.copy()                                                 # :83
        if normb == 0.0:
            normb = 1.0                                               # :85-86
        d0, d1 = _dot(r, r), _dot(rt, r)
        resid = np.sqrt(d0) / normb
        if resid <= tol:
            return 0, 0, resid, x                                     # :88-92
        rho_2 = alpha = omega = 0.0
        p = v = None
        for i in range(1, max_iter + 1):                              # :94
            rho_1 = d1                                                # :95
            if rho_1 == 0:
                return 2, max_iter, np.sqrt(d0) / normb, x            # :96-99
            if i == 1:
                p = r.copy()                                          # :100-101
            else:
                beta = (rho_1 / rho_2) * (alpha / omega)              # :103
                nbo = -beta * omega
                p = 1.0 * r + nbo * v if beta == 0.0 else 1.0 * r + nbo * v + beta * p     # :104
            phat = M(p)                                               # :106
            v = spmv(phat)                                            # :107
            alpha = rho_1 / _dot(v, rt)                               # :108
            s = 1.0 * r + (-alpha) * v                                # :109
            resid = np.sqrt(_dot(s, s)) / normb
            if resid < tol:                                           # :110-115
                x = alpha * phat + 1.0 * x
                return 0, i, resid, x
            shat = M(s)                                               # :116
            t = spmv(shat)                                            # :117
            ts, tt = _dot(t, s), _dot(t, t)
            omega = ts / tt                                           # :118
            x = alpha * phat + omega * shat + 1.0 * x                 # :119
            r = 1.0 * s + (-omega) * t                                # :120
            d0, d1 = _dot(r, r), _dot(rt, r)
            rho_2 = rho_1                                             # :122
            resid = np.sqrt(d0) / normb
            if resid < tol:
                return 0, i, resid, x                                 # :123-127
            if omega == 0:
                return 3, max_iter, resid, x                          # :128-131
        return 1, max_iter, resid, x                                  # :134-135


class State:
    """the state block"""
    def __init__(self):
        self.normb = self.rho = self.rho_next = self.rho_prev = self.alpha = self.omega = self.beta = self.nbo = 0.0
        self.rtv = self.ts = self.tt = self.ss = self.rr = self.resid = self.true_resid = 0.0
        self.it = 0; self.status = -1; self.frozen = 0; self.first = 1; self.half = 0; self.wasted = 0


class BicgstabPlanModel:
    def __init__(self, A, precond=None):
        self.spmv = _spmv_of(A)
        self.M = (lambda v: np.array(v, copy=True)) if precond is None else precond
        self.st = State()
        self.red = [0.0, 0.0]
        self.posts = {}        # ticket -> (it, status, frozen, resid, normb): the ring (no slot is rewritten before it has been read)
        self.seq = 0
        self.info = [0, 0, 0, 0, 0, 0]
        self.p = None

    # ---------------------------------------------------------------- device: scalar steps
    def _post(self):
        self.seq += 1
        s = self.st
        self.posts[self.seq] = (s.it, s.status, s.frozen, s.resid, s.normb)

    def step_normb(self):
        s = self.st
        s.__init__()
        nb = np.sqrt(self.red[0])
        s.normb = nb if nb != 0.0 else 1.0

    def step_init(self, tol, post):
        s = self.st
        s.rr, s.rho_next = self.red
        s.resid = np.sqrt(s.rr) / s.normb
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
        s.rho = s.rho_next
        if s.rho == 0:
            s.frozen, s.status = 1, 2
            return
        if not s.first:
            s.beta = (s.rho / s.rho_prev) * (s.alpha / s.omega)
            s.nbo = -s.beta * s.omega

    def step_alpha(self):
        s = self.st
        if s.frozen:
            return
        s.rtv = self.red[0]
        s.alpha = s.rho / s.rtv

    def step_half(self, tol):
        s = self.st
        if s.frozen:
            return
        s.ss = self.red[0]
        s.resid = np.sqrt(s.ss) / s.normb
        if s.resid < tol:
            s.frozen, s.status, s.half = 1, 0, 1

    def step_omega(self):
        s = self.st
        if s.frozen:
            return
        s.ts, s.tt = self.red
        s.omega = s.ts / s.tt

    def step_res(self, tol, post):
        s = self.st
        s.half = 0
        if not s.frozen:
            s.rr, s.rho_next = self.red
            s.rho_prev = s.rho
            s.first = 0
            s.resid = np.sqrt(s.rr) / s.normb
            if s.resid < tol:
                s.frozen, s.status = 1, 0
            elif s.omega == 0:
                s.frozen, s.status = 1, 3
        if post:
            self._post()

    def step_final(self, iters, tol):
        s = self.st
        s.true_resid = np.sqrt(self.red[0]) / s.normb
        if not s.frozen:
            s.it, s.status = iters, 1
        elif s.status == 0:
            ok = s.true_resid <= tol if s.it == 0 else s.true_resid < tol
            s.status = 0 if ok else 1
        s.frozen = 1

    # ---------------------------------------------------------------- device: vector passes (predicated on the state)
    def pass_p(self):
        s = self.st
        if s.frozen:
            return
        if s.first:
            self.p = self.r.copy()
        elif s.beta == 0.0:
            self.p = 1.0 * self.r + s.nbo * self.v
        else:
            self.p = 1.0 * self.r + s.nbo * self.v + s.beta * self.p

    def pass_s(self):
        s = self.st
        if s.frozen:
            return                      # s and the partials stay; HALF ignores the fold
        self.s = 1.0 * self.r + (-s.alpha) * self.v
        self.red = [_dot(self.s, self.s), 0.0]

    def pass_x(self):
        s = self.st
        if not s.frozen:
            self.x = s.alpha * self.ph + s.omega * self.sh + 1.0 * self.x
        elif s.half:
            self.x = s.alpha * self.ph + 1.0 * self.x

    def pass_r(self):
        s = self.st
        if s.frozen:
            return
        self.r = 1.0 * self.s + (-s.omega) * self.t
        self.red = [_dot(self.r, self.r), _dot(self.rt, self.r)]

    # ---------------------------------------------------------------- the launch sequences
    def enqueue_init(self, tol, post):
        self.red = [_dot(self.b, self.b), 0.0]
        self.step_normb()
        self.r = self.b - self.spmv(self.x)
        self.rt = self.r.copy()
        self.red = [_dot(self.r, self.r), _dot(self.rt, self.r)]
        self.step_init(tol, post)

    def enqueue_iteration(self, it, tol, post):
        """RHO · p-pass · cycle · SpMV with r̃·v · ALPHA · s-pass · HALF · cycle · SpMV with (t·s, t·t) · OMEGA · x-pass · r-pass · RES; a frozen
        iteration runs cycles, SpMVs and the folds all the same"""
        self.step_rho(it)
        self.pass_p()
        self.ph = self.M(self.p)
        self.v = self.spmv(self.ph)
        self.red = [_dot(self.v, self.rt), _dot(self.v, self.v)]
        self.step_alpha()
        self.pass_s()
        self.step_half(tol)
        self.sh = self.M(self.s)
        self.t = self.spmv(self.sh)
        self.red = [_dot(self.t, self.s), _dot(self.t, self.t)]
        self.step_omega()
        self.pass_x()
        self.pass_r()
        self.info[2] += 1
        self.step_res(tol, post)

    def _begin(self, b, x0):
        self.b = np.ascontiguousarray(b, dtype=np.float64)
        self.x = np.zeros(self.b.shape[0]) if x0 is None else np.array(x0, dtype=np.float64)
        self.info[1] += 1
        self.info[2:] = [0, 0, 0, 0]
        if self.p is None or self.p.shape != self.b.shape:      # the plan's vectors are zeroed once, at create
            self.p, self.ph, self.s, self.sh, self.t, self.v, self.r, self.rt = (np.zeros_like(self.b) for _ in range(8))

    # ---------------------------------------------------------------- host: enqueue-only
    def enqueue(self, b, iters, tol, x0=None):
        """→ (status, iterations done, true residual, recursive residual, x); no host look at all"""
        with np.errstate(all="ignore"):
            self._begin(b, x0)
            self.enqueue_init(tol, False)
            for i in range(1, iters + 1):
                self.enqueue_iteration(i, tol, False)
            self.t = self.b - self.spmv(self.x)
            self.red = [_dot(self.t, self.t), 0.0]
            self.step_final(iters, tol)
        s = self.st
        self.info[3] = s.wasted
        return s.status, s.it, s.true_resid, s.resid, self.x

    # ---------------------------------------------------------------- host: the blocking solve
    def _wait(self, ticket):
        self.info[4] += 1
        return self.posts.pop(ticket)

    def solve(self, b, max_iter, tol, ahead, x0=None):
        """→ (status, iterations, resid, x): mgs_bicgstab's contract (iterations = *max_iter on return)"""
        assert ahead >= 0
        with np.errstate(all="ignore"):
            self._begin(b, x0)
            win = min(ahead, RING - 2)
            self.enqueue_init(tol, True)
            out = [(0, self.seq)]            # enqueued, outcome not seen yet
            nxt, seen = 1, -1
            it, status, frozen, resid = 0, -1, 0, 0.0
            while not frozen:
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
                it, status, frozen, resid, _ = self._wait(out.pop(0)[1])
                seen = need
        self.info[3] = self.st.wasted
        if not frozen:
            return 1, max_iter, resid, self.x
        return status, (it if status == 0 else max_iter), resid, self.x
