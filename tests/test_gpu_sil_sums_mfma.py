"""The silhouette cluster sums on the int8 matrix core (sil_sums_mfma) against
the scatter sums they replace (CCG_SIL_SUMS=scatter, read per call) and the
oracle.  Integer sums in any order are the same integers, so every output of
the two paths must agree bit for bit: the means as float64 bit patterns,
nclust and minsize as integers.  The means are also held to the oracle at the
project's 1e-5.

Shapes: the tile is SIL_MT = 512 positions, an MFMA K-step 32 positions, a
cluster block 32 codes, a column tile 32 columns of [d dims | S2 | count]
(d = 30 fills one, d = 31 and 32 take a second), DMAX 16 / 32."""
import concurrent.futures as cf
import os

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-5
T = 512  # SIL_MT


def _both(fn):
    """fn() with the toggle unset (MFMA sums) and with CCG_SIL_SUMS=scatter."""
    old = os.environ.pop("CCG_SIL_SUMS", None)
    try:
        new = fn()
        os.environ["CCG_SIL_SUMS"] = "scatter"
        ref = fn()
    finally:
        os.environ.pop("CCG_SIL_SUMS", None)
        if old is not None:
            os.environ["CCG_SIL_SUMS"] = old
    return new, ref


def _same_bits(a, b):
    for u, v in zip(a, b):
        u, v = np.ascontiguousarray(u), np.ascontiguousarray(v)
        if u.dtype == np.float64:
            assert np.array_equal(u.view(np.uint64), v.view(np.uint64)), (u, v)
        else:
            assert np.array_equal(u, v), (u, v)


def _oracle_means(X, labs):
    """Oracle mean per labeling over the rows whose code is valid (> 0 here:
    the callers mark ignored rows with codes <= 0 after remapping)."""
    out = []
    for lab in labs:
        keep = lab >= 1
        out.append(O.silhouette(X[keep], lab[keep])[1] if keep.any() else np.nan)
    return np.array(out)


def _check_oracle(got, want):
    print("means", got, "oracle", want)
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=1e-12, equal_nan=True)


def _rows_dev(engine, X, labs, cmax):
    """ccg_silhouette_dev (no host-side code check: codes outside [1, cmax] reach the kernels)."""
    import torch
    x = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    lab = torch.from_numpy(np.ascontiguousarray(labs, dtype=np.int32)).cuda()
    L = lab.shape[0]
    mean = torch.empty(L, dtype=torch.float64, device="cuda")
    ncl = torch.empty(L, dtype=torch.int32, device="cuda")
    mns = torch.empty(L, dtype=torch.int32, device="cuda")
    engine.silhouette_t(x, lab, cmax, mean, ncl, mns)
    torch.cuda.synchronize()
    return mean.cpu().numpy(), ncl.cpu().numpy(), mns.cpu().numpy()


def _mixture(rng, m, d):
    centers = rng.normal(scale=3.0, size=(6, d))
    return centers[rng.integers(0, 6, m)] + rng.normal(size=(m, d))


@pytest.mark.parametrize("d", [1, 15, 16, 17, 30, 31, 32])
@pytest.mark.parametrize("m", [1, 31, 33, T - 1, T + 1])
def test_rows_form_bits_and_oracle(engine, m, d):
    rng = np.random.default_rng(1000 * m + d)
    X = _mixture(rng, m, d)
    # cmax = 32 (33 codes with code 0: a second cluster block) and cmax = 255
    for Cs in ((1, 2, 32), (33, 64, 65, 255)):
        labs = np.stack([rng.integers(1, C + 1, m) for C in Cs]).astype(np.int32)
        cmax = max(Cs)
        new, ref = _both(lambda: engine.silhouette(X, labs, cmax=cmax)[:3])
        _same_bits(new, ref)
        _check_oracle(new[0], _oracle_means(X, labs))


@pytest.mark.parametrize("d", [16, 30, 32])
def test_rows_form_ignored_codes_and_empty_code(engine, d):
    """Codes 0, -3 and cmax + 1 are ignored; a code between present ones may be empty."""
    rng = np.random.default_rng(50 + d)
    m, cmax = T + 1, 40
    X = _mixture(rng, m, d)
    a = rng.integers(1, cmax + 1, m)
    a[rng.random(m) < 0.1] = 0
    a[rng.random(m) < 0.1] = -3
    a[rng.random(m) < 0.1] = cmax + 1
    a[-1] = cmax + 1  # (the last position of the second tile)
    b = rng.choice([1, 2, 4, 7, 40], m)  # codes 3, 5, 6, 8 .. 39 empty
    labs = np.stack([a, b]).astype(np.int32)
    new, ref = _both(lambda: _rows_dev(engine, X, labs, cmax))
    _same_bits(new, ref)
    valid = np.where((labs >= 1) & (labs <= cmax), labs, 0)
    _check_oracle(new[0], _oracle_means(X, valid))


def test_limb_extremes(engine):
    rng = np.random.default_rng(77)
    # m = 2: the scale leaves 8 limbs; large and tiny entries of both signs (negative digits, carries)
    X = np.array([[1e6, -1e6, 1e-6, -1e-6, 123456.789], [-1e6, 1e6, -1e-6, 1e-6, -0.5]])
    for labs in (np.array([[1, 1], [1, 2]], np.int32),):
        new, ref = _both(lambda: engine.silhouette(X, labs, cmax=2)[:3])
        _same_bits(new, ref)
        _check_oracle(new[0], _oracle_means(X, labs))
    # every entry negative
    m = 300
    Xn = -np.abs(_mixture(rng, m, 30)) - 0.25
    labs = np.stack([rng.integers(1, C + 1, m) for C in (3, 40)]).astype(np.int32)
    new, ref = _both(lambda: engine.silhouette(Xn, labs, cmax=40)[:3])
    _same_bits(new, ref)
    _check_oracle(new[0], _oracle_means(Xn, labs))
    # all zero: max|x| = 0, scale 2^52
    Xz = np.zeros((100, 7))
    labs = np.stack([rng.integers(1, 4, 100), np.ones(100, np.int64)]).astype(np.int32)
    new, ref = _both(lambda: engine.silhouette(Xz, labs, cmax=3)[:3])
    _same_bits(new, ref)
    _check_oracle(new[0], _oracle_means(Xz, labs))


def test_fewer_than_eight_limbs(engine):
    """m = 70 000: |q| <= 2^61 / m needs 6 limbs, not 8."""
    rng = np.random.default_rng(78)
    m, d = 70000, 5
    X = _mixture(rng, m, d) * 1000.0
    labs = np.stack([rng.integers(1, C + 1, m) for C in (2, 9, 70)]).astype(np.int32)
    new, ref = _both(lambda: engine.silhouette(X, labs, cmax=70)[:3])
    _same_bits(new, ref)
    with cf.ThreadPoolExecutor(3) as ex:
        want = np.array(list(ex.map(lambda lab: O.silhouette(X, lab)[1], labs)))
    _check_oracle(new[0], want)


def _cells_case(rng, d):
    """N = 300 cells, n = 2000 rows; cell 0 has 128 copies and cell 1 has 300
    (weights above 127); labels follow the cell except for a few copies, and
    in some labelings the heavy cells' copies disagree."""
    N, n, L = 300, 2000, 6
    pcs = _mixture(rng, N, d)
    cell = np.concatenate([np.zeros(128, np.int64), np.ones(300, np.int64), rng.integers(2, N, n - 428)])
    rng.shuffle(cell)
    labs = np.empty((L, n), np.int32)
    for l_ in range(L):
        C = (2, 5, 33, 40, 7, 3)[l_]
        lc = rng.integers(1, C + 1, N)
        labs[l_] = lc[cell]
        flip = rng.random(n) < 0.03  # copies labelled apart from their representative
        labs[l_, flip] = rng.integers(1, C + 1, int(flip.sum()))
    r1 = np.flatnonzero(cell == 1)
    r0 = np.flatnonzero(cell == 0)
    # labeling 1: cell 1 splits 200 / 100 (weight still above 127), cell 0 agrees (weight 128)
    labs[1, r1] = 1
    labs[1, r1[-100:]] = 2
    labs[1, r0] = 3
    # labeling 2: cell 1 splits 120 / 180 by its first row's code (weight 120: back on the MFMA)
    labs[2, r1] = 5
    labs[2, r1[:120]] = 4
    return pcs[cell], cell.astype(np.int32), labs, N


@pytest.mark.parametrize("d", [7, 30, 32])
def test_distinct_cells_heavy_weights_and_exceptions(engine, d):
    import torch
    rng = np.random.default_rng(500 + d)
    X, cell, labs, N = _cells_case(rng, d)
    cmax = int(labs.max())
    x = torch.from_numpy(X).cuda()
    lab = torch.from_numpy(labs).cuda()
    cl = torch.from_numpy(cell).cuda()
    L = labs.shape[0]

    def run():
        mean = torch.empty(L, dtype=torch.float64, device="cuda")
        ncl = torch.empty(L, dtype=torch.int32, device="cuda")
        mns = torch.empty(L, dtype=torch.int32, device="cuda")
        engine.silhouette_cells_t(x, lab, cmax, cl, N, mean, ncl, mns)
        torch.cuda.synchronize()
        return mean.cpu().numpy(), ncl.cpu().numpy(), mns.cpu().numpy()
    new, ref = _both(run)
    _same_bits(new, ref)
    _check_oracle(new[0], _oracle_means(X, labs))


def _segments(rng, boots, d, L, C0=2, Cstep=3):
    """As test_gpu_sil_segments builds them; boots: per segment (N cells, the bootstrap's cell of every row)."""
    segs = []
    for s, (N, boot) in enumerate(boots):
        centers = rng.normal(scale=3.0, size=(6, d))
        pop = rng.integers(0, 6, N)
        pcs = centers[pop] + rng.normal(size=(N, d))
        labs = np.empty((L, boot.size), np.int32)
        for l_ in range(L):
            C = C0 + Cstep * (l_ % 8)
            lc = (pop * 3 + l_ + s) % C + 1
            flip = rng.random(N) < 0.1
            lc[flip] = rng.integers(1, C + 1, int(flip.sum()))
            labs[l_] = lc[boot]
        segs.append((pcs[boot], boot, labs, N))
    return segs


def _run_segments(engine, segs, L):
    import torch
    cmax = max(int(s[2].max()) for s in segs)
    ncell = max(s[3] for s in segs)
    off = np.concatenate([[0], np.cumsum([s[0].shape[0] for s in segs])]).astype(np.int64)
    x = torch.from_numpy(np.concatenate([s[0] for s in segs])).cuda()
    cell = torch.from_numpy(np.concatenate([s[1] + q * ncell for q, s in enumerate(segs)]).astype(np.int32)).cuda()
    labels = [torch.from_numpy(s[2]).cuda() for s in segs]
    nseg = len(segs)

    def run():
        means = [torch.full((L,), -7.0, dtype=torch.float64, device="cuda") for _ in range(nseg)]
        ncl = [torch.zeros(L, dtype=torch.int32, device="cuda") for _ in range(nseg)]
        mns = [torch.zeros(L, dtype=torch.int32, device="cuda") for _ in range(nseg)]
        engine.silhouette_segments_t(x, off, labels, cmax, cell, nseg * ncell, means, ncl, mns)
        torch.cuda.synchronize()
        return (np.stack([t.cpu().numpy() for t in means]), np.stack([t.cpu().numpy() for t in ncl]),
                np.stack([t.cpu().numpy() for t in mns]))
    return run


@pytest.mark.parametrize("d", [5, 30])
def test_segments_form(engine, d):
    rng = np.random.default_rng(900 + d)
    L = 12
    boots = []
    for N in (40, 130, 900, 2500, 61, 20):  # (20 cells: 18 rows, under one K-step of 32)
        boots.append((N, rng.integers(0, N, max(2, int(0.9 * N))).astype(np.int32)))
    # exactly T distinct cells: the segment's positions end on a tile boundary
    b = np.concatenate([np.arange(T), rng.integers(0, T, 50)]).astype(np.int32)
    rng.shuffle(b)
    boots.insert(3, (T, b))
    segs = _segments(rng, boots, d, L)
    new, ref = _both(_run_segments(engine, segs, L))
    _same_bits(new, ref)
    jobs = [(q, l_) for q in range(len(segs)) for l_ in range(L)]
    with cf.ThreadPoolExecutor(8) as ex:
        orc = list(ex.map(lambda t: O.silhouette(segs[t[0]][0], segs[t[0]][2][t[1]])[1], jobs))
    _check_oracle(new[0].reshape(-1), np.array(orc))


def test_outside_the_envelope_both_take_the_old_paths(engine):
    rng = np.random.default_rng(5)
    m = 700
    X = _mixture(rng, m, 40)  # d > 32
    labs = np.stack([rng.integers(1, C + 1, m) for C in (3, 20)]).astype(np.int32)
    new, ref = _both(lambda: engine.silhouette(X, labs, cmax=20)[:3])
    _same_bits(new, ref)
    _check_oracle(new[0], _oracle_means(X, labs))
    X = _mixture(rng, m, 12)  # codes past a byte
    labs = np.stack([rng.integers(1, C + 1, m) for C in (3, 300)]).astype(np.int32)
    new, ref = _both(lambda: engine.silhouette(X, labs, cmax=300)[:3])
    _same_bits(new, ref)
    _check_oracle(new[0], _oracle_means(X, labs))


def test_default_run_takes_the_mfma_kernel():
    """The two paths agree bit for bit, so their outputs cannot tell which one
    ran.  Their memory can: only the scatter path allocates the fixed-point
    rows (WS_SIL_Q, m x (DMAX + 1) int64).  A fresh engine per path; the
    device's free memory must drop by those rows more with the toggle set."""
    import torch
    from consensusclustr_amd import Engine
    rng = np.random.default_rng(11)
    m, d, L = 300000, 16, 2
    qbytes = m * (16 + 1) * 8  # 40.8 MB
    x = torch.from_numpy(rng.normal(size=(m, d))).cuda()
    lab = torch.from_numpy(rng.integers(1, 9, (L, m)).astype(np.int32)).cuda()
    mean = torch.empty(L, dtype=torch.float64, device="cuda")
    ncl = torch.empty(L, dtype=torch.int32, device="cuda")
    mns = torch.empty(L, dtype=torch.int32, device="cuda")

    def used():
        eng = Engine(0)
        try:
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info()[0]
            eng.silhouette_t(x, lab, 8, mean, ncl, mns)
            torch.cuda.synchronize()
            return free0 - torch.cuda.mem_get_info()[0], mean.cpu().numpy().copy()
        finally:
            eng.close()
    (u_new, m_new), (u_ref, m_ref) = _both(used)
    print("device bytes taken: default", u_new, "scatter", u_ref, "fixed-point rows", qbytes)
    assert np.array_equal(m_new.view(np.uint64), m_ref.view(np.uint64))
    assert u_ref - u_new >= 0.9 * qbytes


def test_mfma_path_is_deterministic(engine):
    rng = np.random.default_rng(6)
    m = 3 * T + 17
    X = _mixture(rng, m, 30)
    labs = np.stack([rng.integers(1, C + 1, m) for C in (2, 33, 60, 255)]).astype(np.int32)
    old = os.environ.pop("CCG_SIL_SUMS", None)
    try:
        a = engine.silhouette(X, labs, cmax=255)[:3]
        b = engine.silhouette(X, labs, cmax=255)[:3]
    finally:
        if old is not None:
            os.environ["CCG_SIL_SUMS"] = old
    _same_bits(a, b)
