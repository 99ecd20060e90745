"""The device expansion of the SNN class graph into row-level edge lists
(ccg_snn_edges_cells_dev, ccg_snn_edges_stage / ccg_snn_edges_fetch,
Engine.snn_multi(emit="device")): every list equals the oracle's and the host
decoder's bit for bit -- bootstrap copies, rows past the register sort tier,
the capacity protocol, the class-contract fallback and RANK graphs, kNum
handling, back-to-back calls on one stream, tiny and empty rows.
"""
import ctypes

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

SENT_I = -7
SENT_W = -7.0


def _mixture(rng, N, d, C=8, spread=3.0):
    centers = rng.normal(scale=spread, size=(C, d))
    return centers[rng.integers(0, C, N)] + rng.normal(size=(N, d))


def _same(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got, want)) and len(got) == len(want) == 3


def _bufs(torch, caps):
    return [(torch.full((max(c, 1),), SENT_I, dtype=torch.int32, device="cuda"),
             torch.full((max(c, 1),), SENT_I, dtype=torch.int32, device="cuda"),
             torch.full((max(c, 1),), SENT_W, dtype=torch.float64, device="cuda")) for c in caps]


def _untouched(o):
    return bool((o[0] == SENT_I).all() and (o[1] == SENT_I).all() and (o[2] == SENT_W).all())


def _count(engine, torch, knn_t, ks, cl):
    """The count-only call; grows the row reservation when the class rows did
    not fit (the _dev protocol).  Returns d_info as numpy."""
    info = torch.zeros(3 + len(ks), dtype=torch.int64, device="cuda")
    engine.snn_edges_cells_t(knn_t, ks, [None] * len(ks), info, cell=cl)
    torch.cuda.synchronize()
    inf = info.cpu().numpy()
    if inf[3] < 0:
        assert (inf[3:] == -inf[2]).all()
        engine.snn_reserve(int(inf[2]))
        engine.snn_edges_cells_t(knn_t, ks, [None] * len(ks), info, cell=cl)
        torch.cuda.synchronize()
        inf = info.cpu().numpy()
    return inf


def _dev(engine, knn_np, ks, cell=None):
    """Device flavour: count, then fill buffers of exactly the counted sizes.
    Returns ([(i, j, w) numpy per graph], d_info, the device buffers)."""
    import torch
    knn_t = torch.from_numpy(np.ascontiguousarray(knn_np, dtype=np.int32)).cuda()
    cl = None if cell is None else torch.from_numpy(np.ascontiguousarray(cell, dtype=np.int32)).cuda()
    inf = _count(engine, torch, knn_t, ks, cl)
    if inf[1] != 0:
        return None, inf, None
    caps = [int(e) for e in inf[3:]]
    outs = _bufs(torch, caps)
    info = torch.zeros(3 + len(ks), dtype=torch.int64, device="cuda")
    engine.snn_edges_cells_t(knn_t, ks, outs, info, cell=cl, caps=caps)
    torch.cuda.synchronize()
    assert np.array_equal(info.cpu().numpy(), inf)
    got = [tuple(x[:c].cpu().numpy() for x in o) for o, c in zip(outs, caps)]
    return got, inf, outs


@pytest.fixture(scope="module")
def copies_case(engine):
    """test_snn_classes_bootstrap_copies_vs_oracle's input and the oracle's graphs."""
    rng = np.random.default_rng(35)
    N = 5000
    X = _mixture(rng, N, 10)
    X[100:108] = X[7]
    boot = rng.integers(0, N, 4500).astype(np.int32)
    boot[rng.choice(4500, 14, replace=False)] = 3
    boot[rng.choice(4500, 5, replace=False)] = 104
    idx, _ = engine.knn_boot(X, boot, kmax=20)
    knn = np.ascontiguousarray(idx[0])
    return knn, boot, {k: O.snn(knn, k, "number") for k in (10, 15, 20)}


@pytest.mark.parametrize("with_cell", [True, False])
def test_bootstrap_copies(engine, copies_case, with_cell):
    knn, boot, ref = copies_case
    ks = (10, 15, 20)
    cell = boot if with_cell else None
    got, inf, outs = _dev(engine, knn, ks, cell)
    assert inf[1] == 0 and inf[0] < knn.shape[0]
    assert [int(e) for e in inf[3:]] == [ref[k][0].size for k in ks]
    host = engine.snn_multi(knn, list(ks), "number", cell=cell, emit="host")
    for g, k in enumerate(ks):
        assert _same(got[g], ref[k]), k
        assert _same(got[g], host[g]), k
    again, inf2, outs2 = _dev(engine, knn, ks, cell)  # a second identical call: bit-identical buffers
    assert np.array_equal(inf, inf2)
    for a, b in zip(outs, outs2):
        for x, y in zip(a, b):
            assert bool((x == y).all())
    dev = engine.snn_multi(knn, list(ks), "number", cell=cell, emit="device")
    for g, k in enumerate(ks):
        assert _same(dev[g], ref[k]), k


def test_long_rows(engine):
    """A hub matrix: every row lists row 0 first (row 0 lists row 1), so every
    pair shares row 0 and both graphs are complete -- row x has n - 1 - x
    edges, every length from 0 to n - 1.  The register tier ends at 2048
    entries, so n = 3000 reaches the table tier (rows 0 .. 950) and both
    sides of every tier bound (256, 1024, 2048)."""
    rng = np.random.default_rng(7)
    n, k = 3000, 10
    knn = np.empty((n, k), np.int32)
    for i in range(n):
        first = 1 if i == 0 else 0
        pool = np.setdiff1d(np.arange(n, dtype=np.int32), [i, first])
        knn[i, 0] = first
        knn[i, 1:] = rng.choice(pool, k - 1, replace=False)
    ks = (5, 10)
    cell = np.arange(n, dtype=np.int32)
    ref = {kk: O.snn(knn, kk, "number") for kk in ks}
    assert all(ref[kk][0].size == n * (n - 1) // 2 for kk in ks)
    try:
        got, inf, _ = _dev(engine, knn, ks, cell)
        assert inf[1] == 0 and [int(e) for e in inf[3:]] == [n * (n - 1) // 2] * 2
        for g, kk in enumerate(ks):
            assert _same(got[g], ref[kk]), kk
        dev = engine.snn_multi(knn, list(ks), "number", cell=cell, emit="device")
        for g, kk in enumerate(ks):
            assert _same(dev[g], ref[kk]), kk
    finally:
        engine.snn_reserve(0)  # (the hub's class rows needed a larger reservation: back to the default)


def test_capacity_protocol(engine):
    import torch
    from consensusclustr_amd import Engine, _lib
    rng = np.random.default_rng(11)
    N = 3000
    X = _mixture(rng, N, 8)
    idx, _ = engine.knn_boot(X, np.arange(N, dtype=np.int32), kmax=20)
    knn = np.ascontiguousarray(idx[0])
    ks = (10, 20)
    ref = [O.snn(knn, k, "number") for k in ks]
    sizes = [r[0].size for r in ref]
    knn_t = torch.from_numpy(knn).cuda()
    # caps all 0: only the counts
    outs = _bufs(torch, sizes)
    info = torch.zeros(5, dtype=torch.int64, device="cuda")
    engine.snn_edges_cells_t(knn_t, ks, outs, info, caps=[0, 0])
    torch.cuda.synchronize()
    inf = info.cpu().numpy()
    assert inf[1] == 0 and [int(e) for e in inf[3:]] == sizes
    assert all(_untouched(o) for o in outs)
    # graph 0 one short, graph 1 exact: graph 1 is written, graph 0 is not, both counts are reported
    engine.snn_edges_cells_t(knn_t, ks, outs, info, caps=[sizes[0] - 1, sizes[1]])
    torch.cuda.synchronize()
    assert [int(e) for e in info.cpu().numpy()[3:]] == sizes
    assert _untouched(outs[0])
    assert _same(tuple(x.cpu().numpy() for x in outs[1]), ref[1])
    # the host pair: cap too small -> CCG_ECAP; fetch before any stage -> an error, no fault
    ne = (ctypes.c_int64 * 2)()
    karr = (ctypes.c_int * 2)(*ks)
    assert engine.lib.ccg_snn_edges_stage(engine.ctx, knn.ctypes.data_as(ctypes.c_void_p), N, 20, None, karr, 2,
                                          _lib.CCG_SNN_NUMBER, ne) == _lib.CCG_OK
    assert list(ne) == sizes
    ei = np.empty(sizes[0], np.int32)
    p = ei.ctypes.data_as(ctypes.c_void_p)
    assert engine.lib.ccg_snn_edges_fetch(engine.ctx, 0, p, None, None, sizes[0] - 1) == _lib.CCG_ECAP
    assert engine.lib.ccg_snn_edges_fetch(engine.ctx, 0, p, None, None, sizes[0]) == _lib.CCG_OK  # NULL j and w
    assert np.array_equal(ei, ref[0][0])
    assert engine.lib.ccg_snn_edges_fetch(engine.ctx, 2, p, None, None, sizes[0]) == _lib.CCG_EINVAL
    fresh = Engine(0)
    try:
        assert fresh.lib.ccg_snn_edges_fetch(fresh.ctx, 0, p, None, None, sizes[0]) == _lib.CCG_EINVAL
    finally:
        fresh.close()


def test_contract_fallback_and_rank(engine):
    """test_snn_classes_contract_check_and_host_fallback's tight ball: where
    the class contract breaks the device flavour reports status 1 and writes
    nothing; the host pair takes the row-level pass and stays exact; RANK
    graphs go through the row-level emission."""
    import torch
    rng = np.random.default_rng(43)
    N, d = 3000, 8
    X = _mixture(rng, N, d)
    X[200:211] = X[50] + 1e-7 * rng.normal(size=(11, d)) + 500.0
    boot = np.concatenate([np.arange(N), rng.integers(0, N, 600)]).astype(np.int32)
    idx, _ = engine.knn_boot(X, boot, kmax=20)
    knn = np.ascontiguousarray(idx[0])
    ks = (10, 15, 20)
    ref = {k: O.snn(knn, k, "number") for k in ks}
    knn_t = torch.from_numpy(knn).cuda()
    for cell in (None, boot):
        cl = None if cell is None else torch.from_numpy(cell).cuda()
        outs = _bufs(torch, [ref[k][0].size for k in ks])
        info = torch.zeros(6, dtype=torch.int64, device="cuda")
        engine.snn_edges_cells_t(knn_t, ks, outs, info, cell=cl)
        torch.cuda.synchronize()
        inf = info.cpu().numpy()
        if cell is not None:
            assert inf[1] == 0  # the cells keep the ball's points in classes of their own
        if inf[1] == 0:
            for g, k in enumerate(ks):
                assert int(inf[3 + g]) == ref[k][0].size
                assert _same(tuple(x.cpu().numpy() for x in outs[g]), ref[k]), k
        else:
            assert inf[1] == 1 and all(_untouched(o) for o in outs)
        for g, got in enumerate(engine.snn_multi(knn, list(ks), "number", cell=cell, emit="device")):
            assert _same(got, ref[ks[g]]), ks[g]
    for k, got in zip((10, 20), engine.snn_multi(knn, [10, 20], "rank", emit="device")):
        assert _same(got, O.snn(knn, k, "rank")), k


def test_knum_handling(engine):
    rng = np.random.default_rng(5)
    N = 4000
    X = _mixture(rng, N, 10)
    idx, _ = engine.knn_boot(X, np.arange(N, dtype=np.int32), kmax=20)
    ks = (5, 8, 10, 15, 20, 10)  # more than 4 distinct values, one repeated
    host = engine.snn_multi(idx[0], ks, emit="host")
    dev = engine.snn_multi(idx[0], ks, emit="device")
    assert len(dev) == len(host) == len(ks)
    for a, b in zip(dev, host):
        assert _same(a, b)
    with pytest.raises(ValueError):
        engine.snn_multi(idx[0], ks, emit="gpu")
    with pytest.raises(ValueError):
        engine.snn_multi(idx[0], [10], cell=np.zeros(N - 1, np.int32), emit="device")


def test_back_to_back_one_stream(engine):
    """Two bootstraps through the device flavour on one non-default stream,
    nothing between them: the second call's build reuses the workspaces the
    first call's expansion still reads, in stream order."""
    import torch
    rng = np.random.default_rng(21)
    N, n = 3000, 2700
    X = _mixture(rng, N, 10)
    ks = (10, 15, 20)
    cases = []
    for _ in range(2):
        boot = rng.integers(0, N, n).astype(np.int32)
        idx, _ = engine.knn_boot(X, boot, kmax=20)
        knn = np.ascontiguousarray(idx[0])
        cases.append((knn, boot, [O.snn(knn, k, "number") for k in ks]))
    dev = torch.device("cuda", 0)
    knn_t = [torch.from_numpy(c[0]).to(dev) for c in cases]
    cell_t = [torch.from_numpy(c[1]).to(dev) for c in cases]
    outs = [_bufs(torch, [r[0].size for r in c[2]]) for c in cases]
    infos = [torch.zeros(6, dtype=torch.int64, device=dev) for _ in cases]
    engine.snn_edges_cells_t(knn_t[0], ks, [None] * 3, infos[0], cell=cell_t[0])  # (workspaces sized before the run)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        for q in range(2):
            engine.snn_edges_cells_t(knn_t[q], ks, outs[q], infos[q], cell=cell_t[q])
    torch.cuda.synchronize()
    for q in range(2):
        inf = infos[q].cpu().numpy()
        assert inf[1] == 0
        for g in range(3):
            assert int(inf[3 + g]) == cases[q][2][g][0].size
            assert _same(tuple(x.cpu().numpy() for x in outs[q][g]), cases[q][2][g]), (q, g)


def test_tiny_and_empty(engine):
    knn = np.array([[1], [0]], np.int32)  # n = 2, kstride = 1: one edge of weight 2
    ref = O.snn(knn, 1, "number")
    assert ref[0].size == 1 and ref[2][0] == 2.0
    got, inf, _ = _dev(engine, knn, (1,))
    assert inf[1] == 0 and _same(got[0], ref)
    assert _same(engine.snn_multi(knn, [1], emit="device")[0], ref)
    # two disjoint blocks of 20 rows: a block's last row has nothing above it
    rng = np.random.default_rng(3)
    n, k = 40, 5
    knn = np.empty((n, k), np.int32)
    for i in range(n):
        b0 = 20 * (i // 20)
        knn[i] = rng.choice(np.setdiff1d(np.arange(b0, b0 + 20), [i]), k, replace=False)
    ref = O.snn(knn, k, "number")
    assert not np.isin([19, 39], ref[0]).any() and ref[1][ref[0] < 20].max() < 20
    cell = np.arange(n, dtype=np.int32)
    got, inf, _ = _dev(engine, knn, (k,), cell)
    assert inf[1] == 0 and int(inf[3]) == ref[0].size and _same(got[0], ref)
    assert _same(engine.snn_multi(knn, [k], cell=cell, emit="device")[0], ref)
