"""The kNN exact search by radius (knn_fallback_launch: prep, scan, select)
past its two limits, where rows leave the radius search for the per-thread
lists: more than KNN_FX_ROWS = 16 384 failed entries in one call, and more
than KNN_FX_CAP = 1024 candidates for one failed row.  In the segmented batch
(ccg_knn_boots_table_dev) those rows are merged with ids of the concatenation
(knn_fallback_merge_kernel, seg_local = false) and the prep compacts the
entries past the cut too.  Results are held to the oracle's exact scan
(R/consensusClust.R:394 + :656-658: findKNN on pca[sample(...), ]) and, bit
for bit, to the per-bootstrap calls, whose failed lists are far below either
limit.
"""
import os

import numpy as np
import pytest

import oracle as O
from test_gpu_boot_batch import _batch_vs_single, _table

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
FX_ROWS = 16384  # KNN_FX_ROWS


def _short_cells(tab_idx, boots, kq):
    """Per bootstrap, the distinct cells with fewer than kq of their table
    entries present in the bootstrap: the cells the batch sends to the exact
    search (kt_filter_cells_kernel's test, restated on the host)."""
    N = tab_idx.shape[0]
    counts = []
    for b in boots:
        present = np.zeros(N, bool)
        present[b] = True
        cells = np.flatnonzero(present)
        counts.append(int((present[tab_idx[cells]].sum(axis=1) < kq).sum()))
    return np.asarray(counts)


def _assert_batch(engine, torch, pcs, boots, K, kmax, oracle_boots):
    nb, n = boots.shape
    for local_ids in (True, False):
        bi, bd, ri, rd, cut_b, cut_s, rows = _batch_vs_single(engine, torch, pcs, boots, K, kmax=kmax,
                                                              local_ids=local_ids)
        assert np.array_equal(bi, ri)
        assert np.array_equal(bd, rd)
        assert np.array_equal(cut_b, cut_s)
        X_all = rows.cpu().numpy()
        for s in oracle_boots:
            X = X_all[s * n:(s + 1) * n]
            oi, od = O.knn(X, kmax, nthreads=THREADS)
            assert np.array_equal(bi[s * n:(s + 1) * n] - (0 if local_ids else s * n), oi), (s, local_ids)
            np.testing.assert_allclose(bd[s * n:(s + 1) * n], od, rtol=1e-12, atol=1e-12)


def test_segmented_batch_past_the_failed_row_cut(engine):
    """nb = 64 bootstraps of 630 draws from 700 cells, a table of K = 21 for
    kq = 20: a bootstrap holds about 415 distinct cells, each table entry is
    present with p = 0.59, and P(>= 20 of 21 present) is about 2e-4, so nearly
    every distinct cell is short: about 26 000 entries in the compacted list,
    10 000 past the cut.  The count is taken on the host from the table the
    engine returned (itself checked against the oracle) and asserted before
    the batch runs; the per-bootstrap calls have about 415 failures each."""
    import torch
    N, d, nb, K, kmax = 700, 5, 64, 21, 20
    n = 630
    rng = np.random.default_rng(101)
    pcs_np = rng.normal(size=(N, d))
    pcs = torch.from_numpy(pcs_np).to("cuda:0")
    boots = rng.integers(0, N, (nb, n)).astype(np.int32)
    tab_idx, tab_d2 = _table(engine, torch, pcs.t().contiguous(), N, d, K)
    ti, td = tab_idx.cpu().numpy(), tab_d2.cpu().numpy()
    oi, od = O.knn(pcs_np, K, nthreads=THREADS)
    assert np.array_equal(ti, oi)
    np.testing.assert_allclose(np.sqrt(td), od, rtol=1e-12, atol=1e-12)
    short = _short_cells(ti, boots, kmax)
    print("failed distinct cells per bootstrap: min", short.min(), "max", short.max(), "total", short.sum())
    assert short.sum() > FX_ROWS + 4096
    # the bootstrap whose entries straddle entry 16 384 of the compacted list
    # (segment by segment, in bootstrap order)
    ends = np.cumsum(short)
    straddle = int(np.searchsorted(ends, FX_ROWS, side="right"))
    assert 0 < straddle < nb - 1 and ends[straddle - 1] <= FX_ROWS < ends[straddle]
    _assert_batch(engine, torch, pcs, boots, K, kmax, sorted({0, straddle, nb - 1}))


def test_segmented_batch_rows_with_more_than_1024_candidates(engine):
    """Coordinates moved 4096 from the origin: the scan's pre-test allows a
    slack of 2^-14 (|x|^2 + |y|^2), about 1.4e4 at |x|^2 = 7 x 4096^2, against
    squared distances of about 14, so every one of a bootstrap's ~1780
    distinct cells passes for every failed cell: more than KNN_FX_CAP
    candidates, and the row goes to the per-thread lists, which in the batch
    write ids of the concatenation.  K = 21 leaves nearly every distinct cell
    short, about 7100 in all (below the failed-row cut).

    Nothing in the ABI reports the sub-branch.  Confirmed once, on
    2026-10-19, with a build that is not kept and counted in
    knn_fx_select_kernel the entries with a finite radius and a candidate
    count above KNN_FX_CAP: 7130 of the batch's 7130 failed distinct cells
    (of 7133 distinct cells), in both id modes; the per-bootstrap calls'
    1765, 1777, 1810 and 1778 failed cells likewise, all of them."""
    import torch
    N, d, nb, K, kmax = 3000, 7, 4, 21, 20
    n = int(0.9 * N)
    rng = np.random.default_rng(102)
    pcs_np = rng.normal(size=(N, d)) + 4096.0
    pcs = torch.from_numpy(pcs_np).to("cuda:0")
    boots = rng.integers(0, N, (nb, n)).astype(np.int32)
    tab_idx, _ = _table(engine, torch, pcs.t().contiguous(), N, d, K)
    short = _short_cells(tab_idx.cpu().numpy(), boots, kmax)
    uniq = np.array([np.unique(b).size for b in boots])
    print("distinct cells", uniq, "failed distinct cells", short)
    assert (uniq > 1024 + 1).all() and (short > 0.9 * uniq).all() and short.sum() < FX_ROWS
    _assert_batch(engine, torch, pcs, boots, K, kmax, [0, nb - 1])


@pytest.fixture(scope="module")
def copies():
    """20 000 rows drawn from 200 distinct points in 8 dimensions, and the
    oracle's 32 nearest of every row (the order (d2, row) is total, so the 20
    nearest are its first 20 columns)."""
    n, d, npts = 20000, 8, 200
    rng = np.random.default_rng(103)
    pts = rng.normal(size=(npts, d))
    draw = rng.integers(0, npts, n)
    assert np.bincount(draw, minlength=npts).min() > 32 + 1
    X = pts[draw]
    oi, od = O.knn(X, 32, nthreads=THREADS)
    return X, oi, od


@pytest.mark.parametrize("kmax", [20, 32])
def test_rows_call_past_the_failed_row_cut(engine, copies, kmax):
    """ccg_knn_rows_dev on rows with about 100 copies each: the kmax-th and
    the next neighbour tie at distance 0, so certification fails for every
    row; the entries past 16 384 skip the scan and take the per-thread lists
    (lists of 32 at kmax = 32), the others' ~99 candidates at radius 0 the
    select's LDS sort."""
    import torch
    X, oi, od = copies
    n = X.shape[0]
    tr = torch.from_numpy(X).cuda()
    out = torch.full((n, kmax), -1, dtype=torch.int32, device="cuda")
    dist = torch.full((n, kmax), -1.0, dtype=torch.float64, device="cuda")
    queries, fallback = engine.knn_rows_t(tr, kmax, out, out_dist=dist, stats=True)
    torch.cuda.synchronize()
    print("queries", queries, "fallback", fallback)
    assert queries == n
    assert fallback > FX_ROWS
    assert np.array_equal(out.cpu().numpy(), oi[:, :kmax])
    np.testing.assert_allclose(dist.cpu().numpy(), od[:, :kmax], rtol=1e-12, atol=1e-12)
