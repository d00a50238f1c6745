"""The bits of the two block passes (multigridsolver_amd/csrc/blockvec.hip: mgs_vecs_gram, mgs_vecs_combine) against the exact host
restatement tests/eig_ref.py, which tests/test_eig_ref_cpu.py pins.  Equal bits (uint64 views: −0.0 and NaN payloads count), no tolerance.

    n                why
    1                below one pair: the 8-byte path
    63               below a wave
    1030             three workgroups, the last with a tail of three pairs
    1031             the same with an odd last element on one lane
    1 310 723        above the cap of 2048 workgroups: the grid-stride loop runs two to three times per lane (both paths)
    (p, q)           (1, 1) one entry; (8, 8) one full tile; (9, 3) the tile edge plus one; (24, 24) the maximum, nine tiles
    (k, q)           (1, 1); (3, 2); (24, 16) the maximum

Also: the same list on both sides (symmetric bit for bit, tiles below the diagonal mirrored); one column wrapped 8 bytes into a longer
vector (every pass of the call takes the 8-byte path, the same bits as the restatement of that path); integer data whose sums are exact
beside Gaussian data where the order matters; a combine in place; two identical calls; every refusal, and one good call after them."""
import numpy as np
import pytest

import eig_ref as E

pytestmark = pytest.mark.gpu

LENGTHS = (1, 63, 1030, 1031)
INVALID = -1


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


@pytest.fixture(scope="module")
def mg():
    import multigridsolver_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(mg):
    c = mg.Context(0)
    yield c
    c.close()


_DATA = {}


def columns(n, count, kind):
    """`count` columns of length n, made once and left unchanged.  "int": integers in [−8, 8] (every product and sum is exact);
    "gauss": Gaussian entries scaled over five binades (the order of a sum shows in its last bits)"""
    key = (n, count, kind)
    if key not in _DATA:
        rng = np.random.default_rng(1000 * n + 10 * count + (kind == "int"))
        if kind == "int":
            _DATA[key] = [rng.integers(-8, 9, n).astype(np.float64) for _ in range(count)]
        else:
            _DATA[key] = [rng.standard_normal(n) * np.exp2(rng.integers(-2, 3, n)) for _ in range(count)]
    return _DATA[key]


def upload(ctx, cols):
    return [ctx.vec(c) for c in cols]


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("p,q", [(1, 1), (8, 8), (9, 3), (24, 24)])
@pytest.mark.parametrize("n", LENGTHS)
def test_gram_bits(mg, ctx, n, p, q, kind):
    cols = columns(n, p + q, kind)
    U, V = cols[:p], cols[p:]
    vec, nb = E.gram_launch(n)
    G = mg.vecs_gram(upload(ctx, U), upload(ctx, V))
    info = mg.vecs_info(ctx)
    assert info[0] == nb and info[3] == int(vec) and info[5] == 0 and info[6] == 1
    assert info[4] == -(-p // 8) * -(-q // 8) and info[1] == min(p, 8) and info[2] == min(q, 8)
    ref = E.gram(U, V, nb, vec)
    assert same(G, ref)
    if kind == "int":
        assert same(G, np.array(U) @ np.array(V).T + 0.0)


@pytest.mark.parametrize("aligned", [True, False])
def test_gram_capped_grid_stride_path(mg, ctx, aligned):
    """above 2048 workgroups of work the grid is capped and a lane takes several pairs (elements): n = 1 310 723 is 2.5 pairs per lane on the 16-byte
    path and 2.5 elements per lane, from 2048 workgroups, on the 8-byte path"""
    n = 1_310_723
    U, V = columns(n, 3, "gauss")[:2], columns(n, 3, "gauss")[1:]
    dU, dV = upload(ctx, U), upload(ctx, V)
    if not aligned:
        big = ctx.vec(np.concatenate([[0.0], V[0], [0.0, 0.0]]))
        dV[0] = mg.Vec.wrap(ctx, big.ptr + 8, n)
    G = mg.vecs_gram(dU, dV)
    vec, nb = E.gram_launch(n, aligned=aligned)
    info = mg.vecs_info(ctx)
    assert nb == 2048 and info[0] == nb and info[3] == int(vec)
    assert same(G, E.gram(U, V, nb, vec))
    if aligned:
        Gs = mg.vecs_gram(dU, dU)
        assert same(Gs, E.gram(U, U, nb, vec, same=True)) and same(Gs, Gs.T)


@pytest.mark.parametrize("p", [1, 8, 9, 24])
@pytest.mark.parametrize("n", LENGTHS)
def test_gram_same_list_is_symmetric(mg, ctx, n, p):
    U = columns(n, p, "gauss")
    d = upload(ctx, U)
    vec, nb = E.gram_launch(n)
    G = mg.vecs_gram(d, d)
    info = mg.vecs_info(ctx)
    t = -(-p // 8)
    assert info[5] == 1 and info[4] == t * (t + 1) // 2      # tiles on and above the diagonal only
    assert same(G, G.T)
    assert same(G, E.gram(U, U, nb, vec, same=True))
    assert same(G, mg.vecs_gram(d, d))                        # two identical calls


@pytest.mark.parametrize("n", (63, 1030, 1031))
def test_gram_unaligned_column_takes_the_8_byte_path(mg, ctx, n):
    cols = columns(n, 9 + 3, "gauss")
    U, V = cols[:9], cols[9:]
    dU, dV = upload(ctx, U), upload(ctx, V)
    big = ctx.vec(np.concatenate([[0.0], V[1], [0.0, 0.0]]))
    dV[1] = mg.Vec.wrap(ctx, big.ptr + 8, n)                  # 8-byte aligned, not 16
    G = mg.vecs_gram(dU, dV)
    info = mg.vecs_info(ctx)
    vec, nb = E.gram_launch(n, aligned=False)
    assert info[3] == 0 and info[0] == nb and not vec
    assert same(G, E.gram(U, V, nb, False))


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("k,q", [(1, 1), (3, 2), (24, 16)])
@pytest.mark.parametrize("n", LENGTHS)
def test_combine_bits(mg, ctx, n, k, q, kind):
    S = columns(n, k, kind)
    rng = np.random.default_rng(n + k + q)
    Cm = rng.integers(-4, 5, (k, q)).astype(np.float64) if kind == "int" else rng.standard_normal((k, q))
    out = [ctx.vec(np.full(n, np.nan)) for _ in range(q)]
    mg.vecs_combine(upload(ctx, S), Cm, out)
    info = mg.vecs_info(ctx)
    vec, nb = E.combine_launch(n)
    assert info[:4] == [nb, k, q, int(vec)] and info[6] == 2
    ref = E.combine(S, Cm)
    got = [o.numpy() for o in out]
    for j in range(q):
        assert same(got[j], ref[j]), j
    if kind == "int":
        assert np.array_equal(np.array(got).T, np.array(S).T @ Cm)


@pytest.mark.parametrize("n", (63, 1031))
def test_combine_unaligned_and_in_place(mg, ctx, n):
    m = 3
    cols = columns(n, 3 * m, "gauss")                          # X, W, P
    Cm = np.random.default_rng(n).standard_normal((3 * m, 2 * m))
    ref = E.combine(cols, Cm)
    # out of place, one input 8 bytes into a longer vector: the 8-byte path, the same bits
    dS = upload(ctx, cols)
    big = ctx.vec(np.concatenate([[0.0], cols[4], [0.0, 0.0]]))
    dS[4] = mg.Vec.wrap(ctx, big.ptr + 8, n)
    out = [ctx.vec(n) for _ in range(2 * m)]
    mg.vecs_combine(dS, Cm, out)
    assert mg.vecs_info(ctx)[3] == 0
    for j in range(2 * m):
        assert same(out[j].numpy(), ref[j]), j
    # in place, as the eigensolver updates X and P: [X P] ← [X W P]·C
    dS = upload(ctx, cols)
    mg.vecs_combine(dS, Cm, dS[:m] + dS[2 * m:])
    for j in range(m):
        assert same(dS[j].numpy(), ref[j]) and same(dS[2 * m + j].numpy(), ref[m + j]), j
    for j in range(m):
        assert same(dS[m + j].numpy(), cols[m + j])            # W is only read
    # two identical calls
    a, b = [ctx.vec(n) for _ in range(2 * m)], [ctx.vec(n) for _ in range(2 * m)]
    src = upload(ctx, cols)
    mg.vecs_combine(src, Cm, a); mg.vecs_combine(src, Cm, b)
    assert all(same(x.numpy(), y.numpy()) for x, y in zip(a, b))


def test_combine_reads_its_coefficients_before_it_returns(mg, ctx):
    """twenty combines back to back, more than the context's staging slots, the caller's array overwritten with NaN right after every call"""
    n = 1031
    S = columns(n, 3, "gauss")
    dS = upload(ctx, S)
    rng = np.random.default_rng(3)
    Cs = [rng.standard_normal((3, 2)) for _ in range(20)]
    outs = [[ctx.vec(n), ctx.vec(n)] for _ in range(20)]
    buf = np.empty((3, 2))
    for t in range(20):
        buf[:] = Cs[t]
        mg.vecs_combine(dS, buf, outs[t])
        buf[:] = np.nan
    for t in range(20):
        ref = E.combine(S, Cs[t])
        assert same(outs[t][0].numpy(), ref[0]) and same(outs[t][1].numpy(), ref[1]), t


def test_refusals_leave_the_context_working(mg, ctx):
    import ctypes as C
    from multigridsolver_amd._lib import lib
    L = lib()
    n = 100
    cols = columns(n, 4, "gauss")
    d = upload(ctx, cols)
    short = ctx.vec(n - 1)
    H = lambda vs: (C.c_void_p * max(len(vs), 1))(*[v.h if v is not None else None for v in vs])
    G = (C.c_double * 1024)()
    Cm = (C.c_double * 1024)(*([1.0] * 1024))
    many = [d[0]] * 25
    distinct17 = [ctx.vec(n) for _ in range(17)]
    gram = [
        (ctx.h, n, 1, None, 1, H(d), G), (ctx.h, n, 1, H(d), 1, None, G), (ctx.h, n, 1, H(d), 1, H(d), None), (None, n, 1, H(d), 1, H(d), G),
        (ctx.h, n, 1, H([None]), 1, H(d), G),
        (ctx.h, n, 0, H(d), 1, H(d), G), (ctx.h, n, 25, H(many), 1, H(d), G), (ctx.h, n, 1, H(d), 0, H(d), G), (ctx.h, n, 1, H(d), 25, H(many), G),
        (ctx.h, n, 2, H([d[0], short]), 1, H(d), G), (ctx.h, n, 1, H(d), 1, H([short]), G),
        (ctx.h, 0, 1, H(d), 1, H(d), G), (ctx.h, -5, 1, H(d), 1, H(d), G),
    ]
    for args in gram:
        assert L.mgs_vecs_gram(*args) == INVALID, args[1:3]
    out = [ctx.vec(n) for _ in range(2)]
    view = mg.Vec.wrap(ctx, d[0].ptr + 16, n - 2)              # overlaps d[0] without being it
    combine = [
        (ctx.h, n, 1, None, 1, H(out), Cm), (ctx.h, n, 1, H(d), 1, None, Cm), (ctx.h, n, 1, H(d), 1, H(out), None), (None, n, 1, H(d), 1, H(out), Cm),
        (ctx.h, n, 1, H(d), 1, H([None]), Cm),
        (ctx.h, n, 0, H(d), 1, H(out), Cm), (ctx.h, n, 25, H(many), 1, H(out), Cm), (ctx.h, n, 1, H(d), 0, H(out), Cm), (ctx.h, n, 1, H(d), 17, H(distinct17), Cm),
        (ctx.h, n, 2, H([d[0], short]), 1, H(out), Cm), (ctx.h, n, 1, H(d), 1, H([short]), Cm),
        (ctx.h, 0, 1, H(d), 1, H(out), Cm),
        (ctx.h, n, 1, H(d), 2, H([out[0], out[0]]), Cm),        # two outputs that are the same vector
        (ctx.h, n - 2, 1, H(d), 1, H([view]), Cm),              # partial overlap of an output with an input
        (ctx.h, n - 2, 1, H(d), 2, H([out[0], mg.Vec.wrap(ctx, out[0].ptr + 16, n - 2)]), Cm),      # two outputs that overlap
    ]
    for args in combine:
        assert L.mgs_vecs_combine(*args) == INVALID, args[1:5]
    assert L.mgs_vecs_info(ctx.h, None) == INVALID and L.mgs_vecs_info(None, (C.c_int64 * 8)()) == INVALID
    assert all(same(v.numpy(), c) for v, c in zip(d, cols))     # nothing was launched
    vec, nb = E.gram_launch(n)
    assert same(mg.vecs_gram(d, d), E.gram(cols, cols, nb, vec, same=True))
    mg.vecs_combine(d[:2], np.eye(2), out)
    assert same(out[0].numpy(), cols[0]) and same(out[1].numpy(), cols[1])
