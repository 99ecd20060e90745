"""The fused consensus kNN's triangle + candidate-list path (ckc_run and the
COF_CAND epilogue, R/consensusClust.R:421-425), on the branches the scale
tests do not reach.  Every case that claims the candidate path sets
CCG_CKNN_PATH=cand, under which a call that would fall back to the sub-slab
path returns CCG_ECAP instead: a silent fall-back cannot pass for the
candidate path.  Results are held to the oracle's orc_consensus_knn_rows on
sampled rows and, bit for bit, to the sub-slab path (CCG_CKNN_PATH=slab, or a
row-range call, which never takes the candidate path).

* k = 21 and 32: ckc_select_kernel's per-lane lists of 32;
* uint16 labels: one column chunk (the candidate path), and enough slots for
  two (cof_plan's read-back branch cuts; the candidate path declines);
* N = 131 277 > 131 072: the thresholds in two row chunks, the second reusing
  the first launch's slot tables and entry matrix;
* a group of 2049 / 2050 identical cells: 2048 candidates fill a row's list
  exactly, 2049 overflow it; 2048 tied similarities ordered by original id;
* a cell sampled in no column: the NaN flag raised by the candidate epilogue.

N = 33 000 is just above the path's minimum (32 768) and no multiple of the
128 x 256 tile: the last row and column tiles are partial.
"""
import math
import os

import numpy as np
import pytest

import oracle as O
from test_gpu_scale import _robust_A

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
N0, B0 = 33000, 300
CAP = 2048      # CKC_CAP: entries of a row's candidate list
SAMPLE = 4096   # CKC_SAMPLE: the first positions of the row order are the thresholds' sample
NBK = 4096      # CKC_NBK: thresholds are multiples of 1 / NBK


def _orig_of_position(N):
    """ckc_run's row order: the original id of position p is
    (p pmul + padd) mod N.  Used only to state conditions of the inputs (which
    cells are in the sample, which rows the second threshold chunk holds)."""
    pmul = max(2654435761 % N, 2)
    while math.gcd(pmul, N) != 1:
        pmul += 1
    return (np.arange(N, dtype=np.int64) * pmul + N // 3) % N


def _cknn(engine, monkeypatch, At, k, path, r0=0, r1=None):
    """(neighbour matrix, NaN flag) of one device call under CCG_CKNN_PATH =
    path (None: unset).  Rows never written stay -1."""
    import torch
    if path is None:
        monkeypatch.delenv("CCG_CKNN_PATH", raising=False)
    else:
        monkeypatch.setenv("CCG_CKNN_PATH", path)
    N = At.shape[1]
    out = torch.full((N, k), -1, dtype=torch.int32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    engine.consensus_knn_assign_t(At, k, r0, N if r1 is None else r1, out, flag)
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(flag.item())


def _assert_hook_error(engine, monkeypatch, At, k):
    from consensusclustr_amd import CcgError, _lib
    with pytest.raises(CcgError) as e:
        _cknn(engine, monkeypatch, At, k, "cand")
    assert e.value.code == _lib.CCG_ECAP
    assert "CCG_CKNN_PATH=cand" in str(e.value)


def _sample_rows(rng, N, n, extra=()):
    return np.unique(np.concatenate([[0, 1, N - 1], np.asarray(extra, np.int64),
                                     rng.choice(N, n, replace=False)])).astype(np.int32)


def _host16(At):
    return At.cpu().numpy().view(np.uint16)


@pytest.fixture(scope="module")
def base():
    """33 000 cells x 300 robust-path columns (12 populations), on the device."""
    pop = np.random.default_rng(81).integers(0, 12, N0)
    return _robust_A(81, B0, N0, pop)


@pytest.mark.parametrize("k", [21, 32])
def test_k_above_20_runs_the_lists_of_32(engine, monkeypatch, base, k):
    cand, f_c = _cknn(engine, monkeypatch, base, k, "cand")
    slab, f_s = _cknn(engine, monkeypatch, base, k, "slab")
    assert f_c == 0 and f_s == 0
    assert np.array_equal(cand, slab)
    rows = _sample_rows(np.random.default_rng(k), N0, 64)
    ref, nan = O.consensus_knn_rows(base.cpu().numpy(), rows, k, nthreads=THREADS)
    assert not nan.any()
    assert np.array_equal(cand[rows], ref)
    if k == 32:  # the same stable order: a shorter call is a prefix (per-lane lists of 20)
        c10, f10 = _cknn(engine, monkeypatch, base, 10, "cand")
        assert f10 == 0
        assert np.array_equal(c10, cand[:, :10])


def test_hook_refuses_calls_the_candidate_path_does_not_take(engine, monkeypatch, base):
    """A row range, or N below the path's minimum: under `cand` the hook's
    error, not the sub-slab result."""
    from consensusclustr_amd import CcgError, _lib
    for At, r1 in ((base, 128), (base[:, :32000].contiguous(), None)):
        with pytest.raises(CcgError) as e:
            _cknn(engine, monkeypatch, At, 20, "cand", 0, r1)
        assert e.value.code == _lib.CCG_ECAP
        assert "CCG_CKNN_PATH=cand" in str(e.value)


def _wide_A(seed, B, N, pop, top, C=12, pin_max=False, zeros=0.41):
    """_robust_A's columns with every label replaced by a 16-bit code: per
    column an injective random map of its labels into [1, top], flipped cells
    a random code of [1, top].  int16 storage of the uint16 codes (the ABI
    reads any non-uint8 tensor as 16-bit labels).  pin_max: every column's
    largest code is `top`; zeros: the share of cells a column does not sample."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    popt = torch.from_numpy(pop).cuda()
    A = torch.empty((B, N), dtype=torch.int16, device="cuda")
    for b in range(B):
        Cb = int(torch.randint(2, 20, (1,), generator=g, device="cuda").item())
        perm = torch.randperm(C, generator=g, device="cuda") % Cb
        code = torch.randperm(top, generator=g, device="cuda")[:Cb] + 1
        col = code[perm[popt]]
        flip = torch.rand(N, generator=g, device="cuda") < 0.05
        col = torch.where(flip, torch.randint(1, top + 1, (N,), generator=g, device="cuda"), col)
        col[torch.rand(N, generator=g, device="cuda") < zeros] = 0
        if pin_max:
            col[(7919 * b) % N] = top
        A[b] = ((col + 32768) % 65536 - 32768).to(torch.int16)  # the uint16 bit pattern
    return A


def test_uint16_labels_in_one_column_chunk(engine, monkeypatch):
    """Codes up to 1000: (1000 + 8) / 8 = 126 halves per column, 300 columns
    = 37 800, far below a chunk's limit (see the next test), so cof_plan's
    read-back branch returns one chunk and the candidate path completes."""
    k = 20
    pop = np.random.default_rng(82).integers(0, 12, N0)
    At = _wide_A(82, B0, N0, pop, 1000)
    A = _host16(At)
    assert A.max() > 255
    cand, f_c = _cknn(engine, monkeypatch, At, k, "cand")
    slab, f_s = _cknn(engine, monkeypatch, At, k, "slab")
    assert f_c == 0 and f_s == 0
    assert np.array_equal(cand, slab)
    rows = _sample_rows(np.random.default_rng(2), N0, 64)
    ref, nan = O.consensus_knn_rows(A, rows, k, nthreads=THREADS)
    assert not nan.any()
    assert np.array_equal(cand[rows], ref)


def test_uint16_labels_in_two_column_chunks_decline_the_candidate_path(engine, monkeypatch):
    """cof_plan gives a column with largest code m (m + 8) / 8 halves and cuts
    a chunk before the column that would take it past
    cap = 2 max(COF_EMAX / Npad - COF_SLOTS, 4097) halves: with COF_EMAX =
    4 GiB, Npad = 33 000 and COF_SLOTS = 32, cap = 2 (130 150 - 32) =
    260 236.  A column whose largest code is 65 535 takes 8192 halves, so 31
    such columns fit (253 952) and the 32nd does not (262 144): B = 40 columns
    are two chunks, [0, 31) and [31, 40).  ckc_run then returns "not done"
    before its first GEMM.  (10% zeros: at 41% some of the 5e8 pairs would
    share none of only 40 columns, 0.65^40 = 3e-8 each, and the matrix would
    have NaNs.)"""
    k = 20
    B, top = 40, 65535
    npad = (N0 + 3) // 4 * 4
    cap = 2 * max((4 << 30) // npad - 32, 4097)
    per_col = (top + 8) // 8
    assert cap == 260236 and per_col == 8192
    assert 31 * per_col <= cap < 32 * per_col < B * per_col
    pop = np.random.default_rng(83).integers(0, 12, N0)
    At = _wide_A(83, B, N0, pop, top, pin_max=True, zeros=0.1)
    A = _host16(At)
    assert (A.max(axis=1) == top).all()
    _assert_hook_error(engine, monkeypatch, At, k)
    dflt, f_d = _cknn(engine, monkeypatch, At, k, None)
    slab, f_s = _cknn(engine, monkeypatch, At, k, "slab")
    assert f_d == 0 and f_s == 0
    assert np.array_equal(dflt, slab)
    rows = _sample_rows(np.random.default_rng(3), N0, 64)
    ref, nan = O.consensus_knn_rows(A, rows, k, nthreads=THREADS)
    assert not nan.any()
    assert np.array_equal(dflt[rows], ref)


def test_two_threshold_row_chunks(monkeypatch):
    """N = 131 072 + 128 + 77: the thresholds of positions [0, 131 072) and
    [131 072, N) of the row order come from two COF_RECT launches, the second
    with prepared = true.  The oracle checks the rows at the boundary's ids,
    32 random rows on each side, and every row whose position is in the
    second chunk (205 original ids scattered over [0, N)); the sub-slab path,
    called by row range, must equal the first 256 and the last 333 rows bit
    for bit.  96 populations keep every row below 2048 candidates at B = 64
    (about 1100 at most by a CPU estimate; 12 populations overflow).  The call
    takes about 4 GB of workspace: an engine of its own, closed at the end."""
    from consensusclustr_amd import Engine
    R = 131072
    N, B, k = R + 128 + 77, 64, 20
    rng = np.random.default_rng(91)
    pop = rng.integers(0, 96, N)
    At = _robust_A(91, B, N, pop, C=96)
    second = _orig_of_position(N)[R:]
    assert second.size == 205
    rows = _sample_rows(rng, N, 0, extra=np.concatenate([[R - 1, R, R + 1], second, rng.choice(R, 32, replace=False),
                                                         R + rng.choice(N - R, 32, replace=False)]))
    eng = Engine(0)
    try:
        cand, f_c = _cknn(eng, monkeypatch, At, k, "cand")
        assert f_c == 0
        spans = [(0, 256), (R - 128, N)]
        for r0, r1 in spans:
            slab, f_s = _cknn(eng, monkeypatch, At, k, "slab", r0, r1)
            assert f_s == 0
            assert np.array_equal(cand[r0:r1], slab[r0:r1])
    finally:
        eng.close()
    ref, nan = O.consensus_knn_rows(At.cpu().numpy(), rows, k, nthreads=THREADS)
    assert not nan.any()
    assert np.array_equal(cand[rows], ref)


@pytest.fixture(scope="module")
def group():
    """2050 cell ids scattered over [0, N0) in random order, and one column
    pattern for them (labels 1 and 2, 41% zeros)."""
    rng = np.random.default_rng(84)
    ids = rng.choice(N0, CAP + 2, replace=False)
    pat = rng.integers(1, 3, B0).astype(np.uint8)
    pat[rng.random(B0) < 0.41] = 0
    return ids, pat


def _grouped(base, group, M):
    import torch
    ids, pat = group
    gs = np.sort(ids[:M])
    At = base.clone()
    At[:, torch.from_numpy(gs).cuda()] = torch.from_numpy(pat).cuda()[:, None]
    return At, gs


def _assert_group_is_isolated(A, gs, k):
    """The input's conditions: group members agree everywhere they are sampled
    (similarity exactly 1), no other cell reaches (NBK - 2) / NBK with a
    member (so a member's threshold bucket, the top one, admits the group
    only), the sample holds more than k members, and ascending original id is
    not ascending position."""
    N = A.shape[1]
    probe = gs[[0, 1, gs.size // 2, gs.size - 1]].astype(np.int32)
    co, both = O.cocluster_rows(A, probe, nthreads=THREADS)
    co, both = co.astype(np.int64), both.astype(np.int64)
    ing = np.zeros(N, bool)
    ing[gs] = True
    assert (co[:, ing] == both[:, ing]).all() and (both[:, ing] > 0).all()
    assert (co[:, ~ing] * NBK < (NBK - 2) * both[:, ~ing]).all()
    pos = np.empty(N, np.int64)
    pos[_orig_of_position(N)] = np.arange(N)
    gp = pos[gs]
    assert (gp < SAMPLE).sum() > 4 * k
    assert not np.array_equal(np.sort(np.argsort(gp)[:k + 1]), np.arange(k + 1))


def test_candidate_list_filled_exactly_and_ties_by_original_id(engine, monkeypatch, base, group):
    """2049 identical cells: each has the 2048 others as its candidates, all
    at similarity 1 -- slot 2047 is the last that `slot < cap` admits, and the
    selection must order 2048 ties by original id, not by position."""
    k = 20
    At, gs = _grouped(base, group, CAP + 1)
    A = At.cpu().numpy()
    _assert_group_is_isolated(A, gs, k)
    cand, f_c = _cknn(engine, monkeypatch, At, k, "cand")
    slab, f_s = _cknn(engine, monkeypatch, At, k, "slab")
    assert f_c == 0 and f_s == 0
    assert np.array_equal(cand, slab)
    low = gs[:k + 1]
    expect = np.stack([low[low != g][:k] for g in gs])
    assert np.array_equal(cand[gs], expect)
    rows = _sample_rows(np.random.default_rng(4), N0, 48, extra=gs[[0, 1, 7, k, k + 1, gs.size // 2, gs.size - 1]])
    ref, nan = O.consensus_knn_rows(A, rows, k, nthreads=THREADS)
    assert not nan.any()
    assert np.array_equal(cand[rows], ref)


def test_candidate_list_overflow_by_one_falls_back(engine, monkeypatch, base, group):
    """2050 identical cells: 2049 candidates per member, one more than the
    list holds.  The candidate path raises its overflow flag (the hook's
    error); the default call falls back and equals the sub-slab path."""
    k = 20
    At, gs = _grouped(base, group, CAP + 2)
    A = At.cpu().numpy()
    _assert_group_is_isolated(A, gs, k)
    _assert_hook_error(engine, monkeypatch, At, k)
    dflt, f_d = _cknn(engine, monkeypatch, At, k, None)
    slab, f_s = _cknn(engine, monkeypatch, At, k, "slab")
    assert f_d == 0 and f_s == 0
    assert np.array_equal(dflt, slab)
    low = gs[:k + 1]
    assert np.array_equal(dflt[gs], np.stack([low[low != g][:k] for g in gs]))
    rows = _sample_rows(np.random.default_rng(5), N0, 16, extra=gs[[0, k, gs.size - 1]])
    ref, nan = O.consensus_knn_rows(A, rows, k, nthreads=THREADS)
    assert not nan.any()
    assert np.array_equal(dflt[rows], ref)


def test_nan_flag_from_the_candidate_epilogue(engine, monkeypatch, base):
    """A cell sampled in no column has both == 0 with everyone: dbscan's
    stop().  Its row has no usable sampled similarity (tnum = -1) and no
    candidate, nothing overflows, so the candidate path completes and the flag
    is the epilogue's own.  Every other pair is co-sampled, so restoring the
    cell's column clears the flag."""
    k = 20
    c = 12345
    Az = base.clone()
    Az[:, c] = 0
    A = base.cpu().numpy()
    S = (A > 0).astype(np.float32)
    rng = np.random.default_rng(6)
    probe = np.unique(np.concatenate([[0, c, N0 - 1], rng.choice(N0, 512, replace=False)]))
    assert ((S[:, probe].T @ S) > 0).all()  # with c's column in place, the probed rows are co-sampled with every cell
    Sz = S.copy()
    Sz[:, c] = 0
    others = np.arange(N0) != c
    assert ((Sz[:, probe[probe != c]].T @ Sz)[:, others] > 0).all()
    _, f_c = _cknn(engine, monkeypatch, Az, k, "cand")
    _, f_s = _cknn(engine, monkeypatch, Az, k, "slab")
    assert f_c == 1 and f_s == 1
    monkeypatch.setenv("CCG_CKNN_PATH", "cand")
    with pytest.raises(ValueError, match="cannot contain NAs"):
        engine.consensus_knn_assign(Az.cpu().numpy(), k)
    cand, f_c = _cknn(engine, monkeypatch, base, k, "cand")
    slab, f_s = _cknn(engine, monkeypatch, base, k, "slab")
    assert f_c == 0 and f_s == 0
    assert np.array_equal(cand, slab)
    rows = _sample_rows(rng, N0, 16, extra=[c])
    ref, nan = O.consensus_knn_rows(A, rows, k, nthreads=THREADS)
    assert not nan.any()
    assert np.array_equal(cand[rows], ref)
