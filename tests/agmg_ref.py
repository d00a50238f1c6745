"""numpy restatement of the device pairwise aggregation (multigridsolver_amd/csrc/setup_agmg.hip: agg_node_stats_kernel,
agg_edge_weight_kernel, agg_pick_kernel / agg_match_kernel, agg_leader_flag_kernel, agg_assign_kernel, agg_origin_kernel,
agg_zone_kernel, agg_compose_kernel and the chained Galerkin products of k_pairwise_aggregate) — the yardstick of
tests/test_gpu_agmg_matching.py, pinned by tests/test_agmg_ref_cpu.py.

It is NOT oracle.agmg: that is the reference's sequential algorithm (AGMG.cpp:101-315), a different matching.  This module
follows the kernels operation by operation: s_i and the absolute sum are accumulated in ascending column order (over the merged
row/column list when the stored pattern is asymmetric), μ is evaluated exactly as agg_edge_weight_kernel writes it, and the key
order is EdgeKey's (w, distance, parity of mn/(mx−mn), the 32-bit edge_hash, mn — all in origin indices).  The library is built
with -ffp-contract=off, halving is exact and FP64 division is IEEE on both sides, so the device's decisions are expected to be
EQUAL to the ones made here, not close.

Matrices are scipy CSR with sorted columns, rows <= cols (columns >= rows are the halo slots of a row shard); explicitly stored
zeros are part of the pattern and are kept.

The forced last round (round 95: whoever is still undecided becomes a singleton) is restated but exercised by no test: no small
input is known that survives the 71 hash-only rounds before it."""
import numpy as np
import scipy.sparse as sps

MAX_ROUNDS, MU_ROUNDS = 96, 24
# why a directed entry of the matching pattern is not a candidate, in the order the tests are made (each entry counts once)
BRANCHES = ("halo", "g0", "zone", "okay_neg", "zero", "mu_nonpos", "mu_gt_ktg")


def edge_hash(a, b):
    """edge_hash of setup_agmg.hip in 32-bit wrap-around arithmetic; a, b: non-negative ints or arrays → uint32 as int64"""
    M = np.uint64(0xFFFFFFFF)
    a = np.asarray(a).astype(np.uint64) & M
    b = np.asarray(b).astype(np.uint64) & M
    h = ((a * np.uint64(0x9E3779B1)) & M) ^ ((((b + np.uint64(0x7F4A7C15)) & M) * np.uint64(0x85EBCA77)) & M)
    h ^= h >> np.uint64(15); h = (h * np.uint64(0x2C1B3C6D)) & M
    h ^= h >> np.uint64(12); h = (h * np.uint64(0x297A2D39)) & M
    h ^= h >> np.uint64(15)
    return h.astype(np.int64)


def csr(rows, cols, rowptr, col, val):
    """scipy CSR from raw arrays, explicit zeros kept"""
    return sps.csr_matrix((np.asarray(val, dtype=np.float64).copy(), np.asarray(col, dtype=np.int32).copy(), np.asarray(rowptr, dtype=np.int32).copy()),
                          shape=(rows, cols))


def _seq_rowsum(n, rows, vals):
    """Σ per row, the terms added one after the other in the order given (rows ascending)"""
    out = np.zeros(n)
    if rows.size == 0:
        return out
    cnt = np.bincount(rows, minlength=n)
    rank = np.arange(rows.size) - (np.cumsum(cnt) - cnt)[rows]
    order = np.argsort(rank, kind="stable")
    cut = np.searchsorted(rank[order], np.arange(cnt.max() + 1))
    for p in range(cnt.max()):
        sel = order[cut[p]:cut[p + 1]]
        out[rows[sel]] += vals[sel]            # one term per row in each step
    return out


class _Pattern:
    """the matching pattern of A: the union of the stored patterns of A and Aᵀ on the owned columns, plus A's halo entries; equal to
    A's own pattern when that is symmetric.  Per directed entry: row ui, column uj, a_ij and a_ji (0 where not stored; halo: a_ji := a_ij)"""

    def __init__(self, A):
        A = A.tocsr()
        assert A.has_sorted_indices and A.shape[0] <= A.shape[1]
        n, m = A.shape
        nnz = A.nnz
        rows = np.repeat(np.arange(n), np.diff(A.indptr))
        cols = A.indices.astype(np.int64)
        idx = np.arange(1, nnz + 1, dtype=np.int64)
        K = sps.csr_matrix((idx, A.indices.copy(), A.indptr.copy()), shape=(n, m))
        own = cols < n
        KT = sps.csr_matrix((idx[own], (cols[own], rows[own])), shape=(n, m))       # KT[i, j] = K[j, i]
        U = (K + KT * np.int64(nnz + 1)).tocsr(); U.sort_indices()
        kij, kji = U.data % (nnz + 1), U.data // (nnz + 1)
        self.n, self.m = n, m
        self.ui = np.repeat(np.arange(n), np.diff(U.indptr))
        self.uj = U.indices.astype(np.int64)
        vals = np.r_[0.0, A.data]
        self.aij, self.aji = vals[kij], vals[kji]
        self.stored = kij > 0
        halo = self.uj >= n
        self.aji[halo] = self.aij[halo]
        off = self.stored & ~halo & (self.uj != self.ui)
        self.asymmetric = bool(np.any(off & (kji == 0)))                           # pattern_asym_kernel
        assert self.asymmetric or self.stored.all()


def node_stats(pat, ktg, first_pass):
    """agg_node_stats_kernel → (a_ii, s_i, G0)"""
    n = pat.n
    dg = pat.uj == pat.ui
    aii = np.zeros(n); aii[pat.ui[dg]] = pat.aij[dg]
    off = ~dg
    half = (pat.aij[off] + pat.aji[off]) / 2
    ssum = _seq_rowsum(n, pat.ui[off], half)
    asum = _seq_rowsum(n, pat.ui[off], np.abs(half))
    g0 = (aii >= (ktg / (ktg - 2)) * asum) if first_pass else np.zeros(n, dtype=bool)
    return aii, -ssum, g0


def edge_weights(pat, aii, s, g0, ktg, zone=None):
    """agg_edge_weight_kernel → (w per directed entry, +inf = not a candidate; counts per inadmissibility branch; μ as evaluated,
    meaningful where the tests before it passed)"""
    n, ui, uj = pat.n, pat.ui, pat.uj
    todo = uj != ui
    br = {}

    def take(name, mask):
        nonlocal todo
        hit = todo & mask
        br[name] = int(hit.sum())
        todo = todo & ~hit

    take("halo", uj >= n)
    jj = np.where(uj < n, uj, 0)
    take("g0", g0[ui] | g0[jj])
    take("zone", (zone[ui] != zone[jj]) if zone is not None else np.zeros(ui.size, dtype=bool))
    ai, si, aj, sj = aii[ui], s[ui], aii[jj], s[jj]
    take("okay_neg", ~(ai - si + aj - sj >= 0))
    take("zero", (pat.aij == 0.0) & (pat.aji == 0.0))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        num = 2 / (1 / ai + 1 / aj)
        den = (-(pat.aij + pat.aji) / 2) + 1 / (1 / (ai - si) + 1 / (aj - sj))
        mu = num / den
        take("mu_nonpos", ~(mu > 0))
        take("mu_gt_ktg", ~(mu <= ktg))
    w = np.where(todo, mu, np.inf)
    return w, br, mu


def _ids(state):
    """agg_leader_flag_kernel + exclusive scan + agg_assign_kernel"""
    n = state.size
    i = np.arange(n)
    leader = state >= i
    ids = np.cumsum(leader) - leader
    return np.where(state < 0, -1, ids[np.minimum(i, np.maximum(state, 0))]).astype(np.int32), int(leader.sum())


def pairwise_pass(A, ktg, first_pass, origin=None, zone=None):
    """one pass of the device matching on A → (agg int32 with −1 for G0 rows, rounds used, counts per inadmissibility branch)"""
    pat = _Pattern(A)
    n, ui, uj = pat.n, pat.ui, pat.uj
    aii, s, g0 = node_stats(pat, ktg, first_pass)
    w, br, _ = edge_weights(pat, aii, s, g0, ktg, zone)
    org = np.arange(n, dtype=np.int64) if origin is None else np.asarray(origin, dtype=np.int64)
    fin = np.nonzero(np.isfinite(w))[0]
    oi, oj = org[ui[fin]], org[uj[fin]]
    mn, mx = np.minimum(oi, oj), np.maximum(oi, oj)
    assert np.all(mx > mn) and (fin.size == 0 or mn.min() >= 0), "origins of coupled rows must be distinct and non-negative"
    d = mx - mn
    par = (mn // d) & 1
    h = edge_hash(mn, mx)
    fi, fj, fw = ui[fin], uj[fin], w[fin]
    pos = np.arange(fin.size)
    state = np.where(g0, -2, -1).astype(np.int64)
    rounds = 0
    for rnd in range(MAX_ROUNDS):
        hash_only, force = rnd >= MU_ROUNDS, rnd == MAX_ROUNDS - 1
        und = state == -1
        live = pos[und[fi] & und[fj]]
        pick = np.full(n, -1, dtype=np.int64)
        if live.size:
            # smallest key per row; equal keys: the entry met first in storage order (key_less is strict)
            if hash_only:
                order = np.lexsort((live, mn[live], h[live], fi[live]))
            else:
                order = np.lexsort((live, mn[live], h[live], par[live], d[live], fw[live], fi[live]))
            sl = live[order]
            first = np.r_[True, fi[sl][1:] != fi[sl][:-1]]
            pick[fi[sl[first]]] = fj[sl[first]]
        idx = np.nonzero(und)[0]
        p = pick[idx]
        single = p == -1
        mutual = ~single & (pick[np.maximum(p, 0)] == idx)
        rest = ~single & ~mutual
        state[idx[single]] = idx[single]
        state[idx[mutual]] = p[mutual]
        if force:
            state[idx[rest]] = idx[rest]
        rounds = rnd + 1
        if force or not rest.any():
            break
    agg, _ = _ids(state)
    return agg, rounds, br


def galerkin(A, agg):
    """Ā = PᵀAP for the 0/1 aggregation P of agg, as galerkin_lds_kernel forms it: member rows ascending, entries in storage order, every
    entry added to its column's accumulator in the order met; halo column n+k of a shard becomes column nc+k; an entry whose column has
    no aggregate drops out.  Sums that come out as 0 stay in the pattern."""
    n, m = A.shape
    nc = int(agg.max()) + 1 if agg.size else 0
    mc = nc + (m - n)
    cmap = np.r_[agg.astype(np.int64), nc + np.arange(m - n, dtype=np.int64)]
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    c, a = agg[rows].astype(np.int64), cmap[A.indices]
    keep = (c >= 0) & (a >= 0)
    key = c[keep] * mc + a[keep]
    uk, gid = np.unique(key, return_inverse=True)
    val = np.full(uk.size, -0.0)
    np.add.at(val, gid, A.data[keep])            # unbuffered, in index order: the first entry is "stored" (−0.0 + v == v), later ones added
    indptr = np.r_[0, np.cumsum(np.bincount(uk // mc, minlength=nc))]
    return sps.csr_matrix((val, (uk % mc).astype(np.int32), indptr.astype(np.int32)), shape=(nc, mc))


def _min_per_agg(agg, values, nc):
    out = np.full(nc, np.iinfo(np.int64).max)
    sel = agg >= 0
    np.minimum.at(out, agg[sel], values[sel])
    return out


class Aggregation:
    """result of aggregate(): agg (composed ids), origin (per aggregate), A_coarse, and per pass the pass's own agg / rounds / branches /
    the operator it ran on / its zones"""


def aggregate(A, ktg, npass, tou, origin=None, zone=None):
    """k_pairwise_aggregate restated"""
    n = A.shape[0]
    R = Aggregation()
    org = np.arange(n, dtype=np.int64) if origin is None else np.asarray(origin, dtype=np.int64)
    zone = None if zone is None else np.asarray(zone, dtype=np.int64)
    agg, rounds, br = pairwise_pass(A, ktg, 1, org, zone)
    R.passes = [dict(A=A, agg=agg, rounds=rounds, branches=br, zone=zone, first_pass=True)]
    nc = int(agg.max()) + 1
    corg = _min_per_agg(agg, org, nc)
    Abar = galerkin(A, agg)
    for _ in range(2, npass + 1):
        if float(Abar.nnz) <= float(A.nnz) / tou:
            break
        if Abar.shape[0] <= 1:
            break
        czone = None
        if zone is not None:
            czone = np.zeros(Abar.shape[0], dtype=np.int64)
            czone[agg[agg >= 0]] = zone[agg >= 0]
        agg2, rounds, br = pairwise_pass(Abar, ktg, 0, corg, czone)
        R.passes.append(dict(A=Abar, agg=agg2, rounds=rounds, branches=br, zone=czone, first_pass=False))
        nc = int(agg2.max()) + 1
        corg = _min_per_agg(agg2, corg, nc)
        agg = np.where(agg < 0, -1, agg2[np.maximum(agg, 0)]).astype(np.int32)
        Abar = galerkin(Abar, agg2)
    R.agg, R.origin, R.A_coarse, R.nc = agg, corg, Abar, nc
    return R


def pass_counts(agg):
    """(pairs, singletons, G0 rows) of a one-pass agg"""
    sizes = np.bincount(agg[agg >= 0])
    return int((sizes == 2).sum()), int((sizes == 1).sum()), int((agg < 0).sum())


def check_matching(A, agg, ktg, npass=1, first_pass=True, zone=None):
    """Properties of a matching, checked on ALL couplings and without the round logic of pairwise_pass (it shares node_stats and
    edge_weights).  Always: the unaggregated rows are exactly G0 (first pass; none otherwise), ids are the ranks of the aggregates' smallest
    members, sizes <= 2^npass, no aggregate spans two zones.  npass == 1 also: every pair is an admissible coupling (finite μ key in
    (0, ktg]), and no admissible coupling joins two singletons.  Raises AssertionError; returns the counts it saw.

    With npass > 1 this is NOT a full check: admissibility and maximality of the later passes need each pass's own operator and are
    checked by check_passes on the restatement's passes, which says something about a device agg only once that agg has been found
    equal to the restatement's composed ids.  Alone, use it at npass == 1."""
    agg = np.asarray(agg)
    pat = _Pattern(A)
    n = pat.n
    assert agg.shape == (n,)
    aii, s, g0 = node_stats(pat, ktg, first_pass)
    assert np.array_equal(agg < 0, g0), "unaggregated rows != G0"
    rows = np.nonzero(agg >= 0)[0]
    ids, first, sizes = np.unique(agg[rows], return_index=True, return_counts=True)
    nc = ids.size
    assert np.array_equal(ids, np.arange(nc)), "ids are not 0..nc-1"
    assert np.all(np.diff(rows[first]) > 0), "ids are not the ranks of the smallest members"
    assert nc == 0 or sizes.max() <= 2 ** npass, "aggregate larger than 2^npass"
    if zone is not None:
        zone = np.asarray(zone)
        assert np.array_equal(zone[rows], zone[rows[first]][agg[rows]]), "aggregate spans two zones"
    out = dict(aggregates=nc, g0=int(g0.sum()))
    if npass != 1:
        return out
    w, _, _ = edge_weights(pat, aii, s, g0, ktg, zone)
    fin = np.isfinite(w)
    fi, fj = pat.ui[fin], pat.uj[fin]
    size_of = np.zeros(n, dtype=np.int64); size_of[rows] = sizes[agg[rows]]
    left = int(np.sum((size_of[fi] == 1) & (size_of[fj] == 1)))
    assert left == 0, f"{left} admissible couplings join two singletons"
    prow = rows[size_of[rows] == 2]
    order = np.argsort(agg[prow], kind="stable")
    lo, hi = prow[order][0::2], prow[order][1::2]
    assert np.array_equal(agg[lo], agg[hi])
    ok = np.isin(lo.astype(np.int64) * n + hi, fi.astype(np.int64) * n + fj)
    assert ok.all(), f"{int((~ok).sum())} pairs are not admissible couplings, first ({lo[~ok][0]}, {hi[~ok][0]})"
    out.update(pairs=int(lo.size), singletons=int((sizes == 1).sum()), admissible=int(fin.sum()) // 2)
    return out


def check_passes(R, ktg):
    """check_matching on every pass of an aggregate() result (a device agg equal to R.agg is thereby checked pass by pass)"""
    return [check_matching(p["A"], p["agg"], ktg, 1, p["first_pass"], p["zone"]) for p in R.passes]


# ---------------------------------------------------------------------------------------------------------------- inputs of the tests
def chain(n, lo=-1.0, d=2.0, up=-1.0):
    return sps.diags([np.full(n - 1, lo), np.full(n, d), np.full(n - 1, up)], [-1, 0, 1], format="csr")


def chain_closed_form(n):
    """device matching of the uniform chain [−1, 2, −1] (ktg = 10), n >= 5: rows 0 and n−1 are in G0 (2 >= 1.25·1); every interior
    coupling has μ = 2 and distance 1, so the parity rule decides: a node prefers the edge whose lower end is even → pairs (2m, 2m+1) for
    m >= 1 form in round 0.  Row 1 (its even-ended edge goes to G0 row 0) picks row 2 in vain and is a singleton in round 1, with id 0;
    for even n row n−2 is left the same way (its partner n−1 is in G0) and is the last singleton.  Hence agg[i] = i // 2 inside."""
    agg = np.arange(n, dtype=np.int32) // 2
    agg[0] = agg[n - 1] = -1
    return agg


def poisson2d(n):
    T = sps.diags([-np.ones(n - 1), 4 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1])
    S = sps.diags([-np.ones(n - 1), -np.ones(n - 1)], [-1, 1])
    A = (sps.kron(sps.identity(n), T) + sps.kron(S, sps.identity(n))).tocsr(); A.sort_indices()
    return A


def poisson3d(N):
    I = sps.identity(N)
    S = sps.diags([-np.ones(N - 1), -np.ones(N - 1)], [-1, 1])
    A = (6 * sps.identity(N ** 3) + sps.kron(sps.kron(S, I), I) + sps.kron(sps.kron(I, S), I) + sps.kron(sps.kron(I, I), S)).tocsr()
    A.sort_indices()
    return A


def poisson3d_shard(N, p0, p1):
    """rows of the planes p0..p1−1 of poisson3d(N) with local columns: the owned rows first, then the halo slots rows + k, the columns
    of plane p0−1 followed by those of plane p1, each in ascending order (0 < p0 < p1 < N) → (A with rows < cols, zones: first owned
    plane 1, last owned plane 2, interior 0)"""
    assert 0 < p0 < p1 < N
    pl = N * N
    rows = (p1 - p0) * pl
    S = poisson3d(N)[p0 * pl:p1 * pl].tocsc()
    A = sps.hstack([S[:, p0 * pl:p1 * pl], S[:, (p0 - 1) * pl:p0 * pl], S[:, p1 * pl:(p1 + 1) * pl]]).tocsr(); A.sort_indices()
    zone = np.zeros(rows, dtype=np.int32); zone[:pl] = 1; zone[-pl:] = 2
    return A, zone


def random_nonsymmetric(n=3000, seed=11, margin=0.02):
    """random sparse graph, symmetric pattern, a_ij != a_ji, all weights distinct; rows dominant by `margin` of the symmetric part"""
    rng = np.random.default_rng(seed)
    r = np.r_[np.arange(n - 1), rng.integers(0, n, 2 * n)]
    c = np.r_[np.arange(1, n), rng.integers(0, n, 2 * n)]
    keep = r != c
    Pm = sps.csr_matrix((np.ones(keep.sum()), (r[keep], c[keep])), shape=(n, n)); Pm = ((Pm + Pm.T) > 0).tocsr(); Pm.sort_indices()
    W = Pm.astype(np.float64); W.data = rng.random(W.nnz) + 0.2
    S = (W + W.T) * 0.5
    dg = np.asarray(S.sum(axis=1)).ravel() * (1 + margin * rng.random(n)) + 0.01 * rng.random(n)
    A = (sps.diags(dg) - W).tocsr(); A.sort_indices()
    return A


def _entry(A, i, j):
    k = A.indptr[i] + np.searchsorted(A.indices[A.indptr[i]:A.indptr[i + 1]], j)
    assert A.indices[k] == j
    return k


def mu_of(A, ktg, i, j):
    """μ({i,j}) as the restatement evaluates it for the stored entry (i, j), whatever its admissibility"""
    pat = _Pattern(A)
    aii, s, g0 = node_stats(pat, ktg, True)
    return edge_weights(pat, aii, s, g0, ktg)[2][np.nonzero((pat.ui == i) & (pat.uj == j))[0][0]]


def branchy(n=1200, seed=5, ktg=10.0):
    """random_nonsymmetric changed so that the restatement takes every inadmissibility branch of a square, zone-free input: positive
    couplings with a_ij + a_ji > 0 (μ <= 0), neighbouring rows with s_i > a_ii (a_ii − s_i + a_jj − s_j < 0), couplings stored as zero
    on both sides, strongly dominant rows (G0), and two couplings −t (both sides) with t found by bisection down to neighbouring
    doubles: at the first edge returned the largest t whose μ is still > ktg, at the second the smallest t whose μ is <= ktg (the edges
    are the first two of (100, 101), (150, 151), ... whose μ can cross ktg at all).  → (A, [edge above, edge below])"""
    rng = np.random.default_rng(seed)
    A = random_nonsymmetric(n, seed, margin=0.3)
    cand = np.arange(100, n - 100, 50)
    free = np.setdiff1d(np.arange(n - 1), (cand[:, None] + np.arange(-5, 6)).ravel())

    def put(i, j, v):
        A.data[_entry(A, i, j)] = v

    for i in rng.choice(free, 40, replace=False):                 # positive couplings
        put(i, i + 1, 0.9); put(i + 1, i, 0.7)
    for i in rng.choice(free, 40, replace=False):                 # stored zeros on both sides
        put(i, i + 1, 0.0); put(i + 1, i, 0.0)
    for i in rng.choice(free, 30, replace=False):                 # neighbouring rows with s_i > a_ii
        A.data[_entry(A, i, i)] *= 0.8; A.data[_entry(A, i + 1, i + 1)] *= 0.8
    for i in rng.choice(free, 60, replace=False):                 # G0 rows
        A.data[_entry(A, i, i)] *= 3
    edges = []
    for i in cand:
        j = i + 1

        def mu(t):
            put(i, j, -t); put(j, i, -t)
            return mu_of(A, ktg, i, j)
        lo, hi = 1e-3, 1.0
        if not (mu(lo) > ktg >= mu(hi) > 0):
            continue
        while np.nextafter(lo, hi) < hi:
            mid = 0.5 * (lo + hi)
            if mu(mid) > ktg:
                lo = mid
            else:
                hi = mid
        mu(hi if edges else lo)
        edges.append((int(i), int(j)))
        if len(edges) == 2:
            break
    assert len(edges) == 2
    return A, edges


def hash_chain(n=120):
    """tridiagonal, couplings c_i = 1 + 0.01·i, diagonal c_{i−1} + c_i + 0.05: the weights fall monotonically along the chain, each μ round
    pairs only the locally dominant end, and the 24 μ rounds run out"""
    c = 1 + 0.01 * np.arange(n - 1)
    dg = np.r_[0.0, c] + np.r_[c, 0.0] + 0.05
    return sps.diags([-c, dg, -c], [-1, 0, 1], format="csr")


def one_sided_random(n=1500, seed=3):
    """the operator of test_pattern_asymmetric_operator_setup: forward-only chain plus random one-directional links, M-matrix"""
    rng = np.random.default_rng(seed)
    rows = np.r_[np.arange(n - 1), rng.integers(0, n, 2 * n)]
    cols = np.r_[np.arange(1, n), rng.integers(0, n, 2 * n)]
    keep = rows != cols
    W = sps.csr_matrix((rng.random(keep.sum()) + 0.2, (rows[keep], cols[keep])), shape=(n, n)); W.sum_duplicates()
    d = np.maximum(np.asarray(W.sum(axis=1)).ravel(), np.asarray(W.sum(axis=0)).ravel()) * 1.02 + 0.01
    A = (sps.diags(d) - W).tocsr(); A.sort_indices()
    return A


def forward_chain(n=301):
    """only a_{i,i+1} is stored; weights 1 + (7·i mod 13)/13 (ties and non-ties), diagonal 1.1 × the larger of row and column sum"""
    c = 1 + (7 * np.arange(n - 1) % 13) / 13
    dg = 0.55 * (np.r_[c, 0.0] + np.r_[0.0, c]) + 0.01
    A = (sps.diags(dg) - sps.diags(c, 1)).tocsr(); A.sort_indices()
    return A


def one_sided_zeros(n=24, seed=2):
    """2-D Poisson whose pattern stays symmetric while a third of the couplings are a stored ZERO on one side (−2 on the other)"""
    rng = np.random.default_rng(seed)
    A = poisson2d(n).tocoo()
    up = np.nonzero(A.row < A.col)[0]
    hit = rng.choice(up, up.size // 3, replace=False)
    data = A.data.copy()
    data[hit] = 0.0
    lo = {(int(c), int(r)) for r, c in zip(A.row[hit], A.col[hit])}
    for k in np.nonzero(A.row > A.col)[0]:
        if (int(A.row[k]), int(A.col[k])) in lo:
            data[k] = -2.0
    order = np.lexsort((A.col, A.row))
    r, c, v = A.row[order], A.col[order], data[order]
    return sps.csr_matrix((v, c.astype(np.int32), np.r_[0, np.cumsum(np.bincount(r, minlength=n * n))].astype(np.int32)), shape=(n * n, n * n))
