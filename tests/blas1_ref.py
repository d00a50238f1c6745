"""Exact host restatement of the BLAS-1 reductions and updates (multigridsolver_amd/csrc/blas1.hip, blas1.hpp), numpy only: the launch
arithmetic, the order in which every lane adds its terms, the workgroup fold, the middle and the last stage.  Every addition below is one
IEEE double addition on arrays (no Python loop over elements), in the order the kernels perform it, so the results carry the kernels' bits.
tests/test_blas1_ref_cpu.py pins this file; tests/test_gpu_blas1_bits.py holds the device to it.

`defect` plants one wrong order, for the tests that show the fixtures can tell: "tail_first" (the odd last element added before the pairs),
"wave_from_first" (the wave sums started from the first wave's sum, not from 0.0), "no_mid" (long partial arrays folded without the
middle stage)."""
import numpy as np

TB = 256                # lanes per workgroup
DOT_BLOCKS = 4096       # partial slots of the context's scratch; a pass with partial pairs uses half per sum
MID_ABOVE = 4096        # more partials than this: 256 chunk sums first
MID_GROUPS = 256


# ------------------------------------------------------------------------------------------------------------- launch arithmetic
def cdiv(a, b):
    return -(-a // b)


def grid_vec(n2, pairs, n_cu):
    """workgroups of a 16-byte launch over n2 pairs: blas1_pairs = k > 0 pairs per lane, 0: the capped grid of 8 workgroups per CU"""
    g = cdiv(n2, TB)
    if pairs > 0:
        return max(1, cdiv(g, pairs))
    return max(1, min(g, n_cu * 8))


def grid_cap(n, cap):
    """workgroups of an 8-byte grid-stride launch: one lane per entry, at most cap, at least one"""
    return max(1, min(cdiv(n, TB), cap))


def dot_launch(n, aligned=True, blas1_vec=1, blas1_pairs=1, n_cu=256):
    """k_dot → (16-byte form?, workgroups)"""
    if blas1_vec and n >= 2 and aligned:
        return True, grid_vec(n // 2, blas1_pairs, n_cu)
    return False, grid_cap(n, DOT_BLOCKS)


def project_launch(n, aligned=True, blas1_vec=1, blas1_pairs=1, n_cu=256):
    """k_project_const* → (16-byte form?, workgroups); both of its passes use this grid"""
    if blas1_vec and aligned:
        return True, grid_vec((n + 1) // 2, blas1_pairs, n_cu)
    return False, grid_cap(n, DOT_BLOCKS // 2)


def mid_chunk(nb):
    """entries per workgroup of the middle stage, or 0 where the last stage folds the partials itself"""
    return cdiv(nb, MID_GROUPS) if nb > MID_ABOVE else 0


# ------------------------------------------------------------------------------------------------------------------- the folds
def lane_sums(p, nb, vec, defect=None):
    """[nb][TB] lane sums of the terms p, each from 0.0.  16-byte form: lane t of workgroup b adds p[2i], then p[2i + 1], for
    i = b·TB + t stepping by nb·TB; the odd last term is added last, on lane 0 of workgroup 0.  8-byte form: p[i], same stepping."""
    p = np.asarray(p, dtype=np.float64)
    n, L = len(p), nb * TB
    s = np.zeros(L)
    if not vec:
        for k in range(0, n, L):
            c = p[k:k + L]
            s[:len(c)] += c
        return s.reshape(nb, TB)
    n2 = n // 2
    if defect == "tail_first" and n & 1:
        s[0] += p[n - 1]
    p0, p1 = p[0:2 * n2:2], p[1:2 * n2:2]
    for k in range(0, n2, L):
        m = min(L, n2 - k)
        s[:m] += p0[k:k + m]
        s[:m] += p1[k:k + m]
    if defect != "tail_first" and n & 1:
        s[0] += p[n - 1]
    return s.reshape(nb, TB)


def workgroup_fold(s, defect=None):
    """[nb][TB] lane values → nb workgroup sums: six shuffle levels inside each wave of 64, then the four wave sums in wave order from 0.0"""
    w = np.array(s, dtype=np.float64).reshape(-1, TB // 64, 64)
    off = 32
    while off:
        w[..., :off] += w[..., off:2 * off]
        off >>= 1
    t = w[:, 0, 0].copy() if defect == "wave_from_first" else np.zeros(w.shape[0]) + w[:, 0, 0]
    for q in range(1, TB // 64):
        t += w[:, q, 0]
    return t


def mid_fold(part):
    """dot2_mid_kernel on one partial array: MID_GROUPS chunk sums; workgroup g adds part[g·chunk + t], stepping by TB inside its chunk"""
    nb = len(part)
    chunk = mid_chunk(nb)
    steps = cdiv(chunk, TB)
    padded = np.zeros(MID_GROUPS * chunk)
    padded[:nb] = part
    live = np.arange(MID_GROUPS * chunk).reshape(MID_GROUPS, chunk) < nb
    padded = padded.reshape(MID_GROUPS, chunk)
    s = np.zeros((MID_GROUPS, TB))
    for k in range(steps):
        c, m = padded[:, k * TB:(k + 1) * TB], live[:, k * TB:(k + 1) * TB]
        width = c.shape[1]
        s[:, :width] = np.where(m, s[:, :width] + c, s[:, :width])
    return workgroup_fold(s)


def final_fold(part):
    """the last stage: lane t adds part[t], part[t + TB], ... from 0.0, then a TB-wide tree in LDS; sh[0]"""
    part = np.asarray(part, dtype=np.float64)
    sh = np.zeros(TB)
    for k in range(0, len(part), TB):
        c = part[k:k + TB]
        sh[:len(c)] += c
    w = TB // 2
    while w:
        sh[:w] += sh[w:2 * w]
        w >>= 1
    return float(sh[0])


def staged_fold(part, defect=None):
    """k_dot2_finish on one partial array: the middle stage above MID_ABOVE partials, then the last stage"""
    if mid_chunk(len(part)) and defect != "no_mid":
        part = mid_fold(part)
    return final_fold(part)


def reduce_terms(p, nb, vec, defect=None):
    """one whole reduction of the terms p: lanes, workgroups, staged fold"""
    return staged_fold(workgroup_fold(lane_sums(p, nb, vec, defect), defect), defect)


# ------------------------------------------------------------------------------------------------------------------ the results
def dot(x, y, defect=None, **launch):
    """mgs_dot; launch: aligned, blas1_vec, blas1_pairs, n_cu"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    vec, nb = dot_launch(len(x), **launch)
    return reduce_terms(x * y, nb, vec, defect)


def nrm2(x, **launch):
    """mgs_nrm2: the square root (correctly rounded) of mgs_dot(x, x)"""
    return float(np.sqrt(dot(x, x, **launch)))


def project_const(v, **launch):
    """mgs_vec_project_const with the norm → (sum, m = sum/n, v − m, ‖v − m‖² as folded, its square root)"""
    v = np.asarray(v, dtype=np.float64)
    n = len(v)
    vec, nb = project_launch(n, **launch)
    total = reduce_terms(v, nb, vec)
    m = float(np.float64(total) / np.float64(n))
    o = v - m
    q = reduce_terms(o * o, nb, vec)
    return total, m, o, q, float(np.sqrt(q))


def axpby(a, x, b, y):
    """mgs_axpby, element i: a·x_i + b·y_i; b == 0: a·x_i, y is not read"""
    a, b = np.float64(a), np.float64(b)
    return a * x if b == 0.0 else a * x + b * y


def axpbypcz(a, x, b, y, c, z):
    """mgs_axpbypcz, element i: a·x_i + b·y_i + c·z_i, added left to right; c == 0: a·x_i + b·y_i, z is not read"""
    a, b, c = np.float64(a), np.float64(b), np.float64(c)
    return a * x + b * y if c == 0.0 else a * x + b * y + c * z
