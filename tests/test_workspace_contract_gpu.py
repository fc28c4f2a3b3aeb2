"""The "Caller memory" contract of include/statdepth_hip.h on the device: every compute entry point, on every route its plan
names, with the workspace and the outputs replaced by guarded buffers of exactly the promised size that hold 0x00, 0xFF
or 0xA5 on entry (tests/workspace_contract.py).  Per case: the guards are intact, the results hold the same bits under
the three poisons and on the caller's own buffers, and they agree with the family's CPU reference under the family's own
criterion.  Then the gate words of the two rank routes that are never zeroed, against workspaces full of the very word
that reads as "set" (fresh copies of the library, whose epoch counters start at 0).

Its last test asserts that the proxy saw every symbol of the table under every poison, whenever the whole module ran in
the process.

Carve-out -> what initialises it before its first read (read from the sources before the first poisoned run; "run": the
cases below are what shows it)
---------------------------------------------------------------------------------------------------------------------
sd_api.hip        time-major copy Yw (every curve family)      the transpose launch at the head of the call writes all T n
                  nan_cnt[T] (sd_mbd_counts, external)         the counting launch stores every entry (=)
                  part (sd_mbd_counts_wide)                    the inner call's out; wide_add_kernel `first` stores =
mbd_rank_ab       partial blocks (BucketFold)                  every workgroup of the bucket kernel stores its whole block
                  AB, nnan (PairImage, MediumImage)            the image launch stores every (row, curve) and row
mbd_rank_bucket   two-launch path: P32 blocks                  rank_bucket32_kernel, every workgroup, all n entries
                  rowflag[rows]                                rank_bucket32_kernel: = per ranked row; the rows a workgroup
                                                               leaves behind (stop, hand-over) are set to 1 before it ends
                  gate[0] (flagged), gate[1] (contenders)      NOT initialised: "set" means == the call's epoch
                  gate[2] (arrival counter `done`)             rank_bucket32_kernel, workgroup 0 thread 0, = 0 at its start
                  fblocks (second launch)                      the SEL form rewrites `rows` to nsel, the number of flagged
                                                               rows, before anything else; flagged row r goes to workgroup
                                                               r % G, so exactly the first min(nsel, G) workgroups own one,
                                                               store their block, and only those blocks are read
                  all-totals (target subsets)                  out_zero of the first launch, = 0 by every workgroup
                  out (two-launch path adds with atomics)      rank_bucket32_kernel zeroes out on the first batch
mbd_rank_big      bcnt, bflag, nnanrow, ovf, nanf (`zero`)     bucket_setup_kernel (S3) per row of every batch, = 0
                  meet[2 + 1024]                               S3, the workgroup of row 0, every batch, = 0
                  rowtied, spl, mk, tab, rp                    S3 stores them per row
                  gate[0], gate[1]                             NOT initialised: "set" means == the batch's epoch
                  bval, bidx, sorted, AB2 image                the partition / rank / sort launches store what is read
                                                               (within bcnt, ovf and the chunk lengths)
bd_strict         out                                          hipMemsetAsync at the head of the call (atomics add to it)
                  tiemask, cmask, xnan, dflag, dirty, dcount   hipMemsetAsync before their first kernel
                  hash table keys / cnt                        the clear kernel in front of strict_match_insert_kernel
                  `none`, NaN flag                             hipMemsetAsync (0xFF / 0)
                  masks, HF, meta                              run (the mask kernels store per target and curve)
bd_strict_class   flag                                         hipMemsetAsync(flag, 0, 4)
bd_strict_grid    cursor, cellcnt, hc, cnt, slot               hipMemsetAsync each;  R, nnan, rec, start and the nested
                                                               large-n scratch: run (test_strict_grid_and_rank32)
band_enum         Y, AB                                        run;  out: hipMemsetAsync
mbd_pairwise      out                                          hipMemsetAsync
rank_depths       AB / u64 image, nnan                         the image launch of the batch; out: = on the first batch
extremal          E[n][T], H[n]                                the transform of every batch stores E; the sort stores H;
                                                               out: hipMemsetAsync (atomics add to it)
tvd               part[m][16][4] (slice records)               tvd_fold_kernel / tvd_pairwise_kernel store every (target,
                                                               slice) record, = on the batch with row0 == 0
                  carry[n]                                     hipMemcpyAsync behind every batch that has a successor;
                                                               read only at r == 0 of a batch with row0 > 0
                  C[rows][n]                                   tvd_dominance_kernel for every row pair of the batch
multi_cloud       Y, V, extra (Cn) per batch                   the projection launches; V: hipMemsetAsync per batch
                  out (records)                                the fold with first = (t0 == 0) stores =
directional_out   Cn[tb], centres, curves                      do_centre_kernel stores every timepoint; do_moments_kernel
                                                               every (target, t, e); records = on the first batch
halfspace         K, I, part (sort), cnt                       cnt: hipMemsetAsync 0xFF; acc: hipMemsetAsync;  sort: run
halfspace_exact   out                                          hipMemsetAsync 0xFF (minima)
simplicial_exact, simplex, oja, prob_*, lens: out              hipMemsetAsync 0 (atomics / sums add to it)
projection        med, mad per chunk                           run;  out: hipMemsetAsync for external targets
central_regions   ws_fence, ws_outside, partial                counts: hipMemsetAsync; the rest run
curve_dist        hmodal part                                  the tile launch stores every (target, tile) sum
                  select hist, state                           cd_select_init_kernel;  slab: the tile launch stores n x n
spatial_depth     W, F                                         the weight launch and the sum launch of the batch
lens_depth        D (n x n), A (rows of a batch)               the tile launches store every entry

Waits on other workgroups (searched: every atomic load and sleep of the sources): rank_bucket_kernel's SEL tail waits for
`done` == G -- every workgroup of that launch takes a ticket (the early return in front of it depends on *gate alone, which
no workgroup of the second launch writes, so either all return or none does) and `done` is zeroed by the first launch;
big_fallback_kernel's meeting is bounded by spin_limit with take-over and its words are zeroed by S3.  bd_strict's two
atomic loads are bounded probes of a hash table.

The stale gates, from the code: a stale gate[0] == epoch (both routes) makes the second launch / the fall-back kernel scan
flags that the first launch of the same batch has written -- time, never results.  A stale gate[1] == epoch on the large-n
route scans ovf[], zeroed by S3 -- the same.  A stale gate[1] == epoch << 8 | (count >= 8) on the two-launch path made
every workgroup leave its remaining rows to the second launch WITHOUT opening gate[0] when none of its own rows was bad:
the second launch returned at once and those rows were lost.  Fixed in rank_bucket32_kernel (a workgroup that stops
opens the gate); test_stale_gate_words_of_the_two_launch_path is the case.

References.  Integers and the families specified bit for bit (spatial sums included) are compared exactly with their
modules' restatements.  L1 depths, the h-modal sums, the doubles of TVD, the Oja volume sums and the probabilistic sums are
held to their modules' own bounds against those modules' references (l1_tolerance, hmodal_bound, check_doubles, 1e-12
of assert_depths_close, 1e-12 / 1e-13 / 1e-10 relative)."""
import contextlib
import functools
import math
import shutil

import numpy as np
import pytest

from statdepth_amd import _native
from test_boxplot_host import boxplot_np
from test_curve_dist_host import sqdist_exact
from test_directional_host import multi_outlyingness_records
from test_extremal_host import extremal_counts_lexsort
from test_halfspace_exact_host import exact_counts, exact_external, integer_cloud
from test_halfspace_host import halfspace_counts_sorted, halfspace_external, make_directions
from test_curve_dist_gpu import check_sums
from test_l1_host import l1_errors, l1_reference, l1_tolerance
from test_lens_depth_host import lens_counts_np
from test_multi_cloud_host import multi_halfspace_records, multi_projection_records
from test_oja_host import oja_sums
from test_probabilistic_band_host import band_sums
from test_probabilistic_host import normal_sums, poisson_sums
from test_projection_host import projection_external, projection_outlyingness
from test_rank_depths_host import records_np
from test_simplicial_exact_host import simplicial_counts, simplicial_external
from test_spatial_depth_host import spatial_exact
from test_tvd_gpu import check_doubles
from test_tvd_host import tvd_counts_np
from conftest import assert_depths_close
from workspace_contract import OUTPUTS, POISONS, ContractProxy, Memory, compute_symbols

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


@pytest.fixture(scope="module")
def seen():
    """What the module's proxies saw in this process: (symbol, poison) of every guarded call, and the test functions that ran."""
    return {"calls": set(), "tests": set()}


@pytest.fixture
def poisoned(monkeypatch, eng, seen, request):
    """with poisoned(0xA5): the engine runs on the product library behind the contract proxy."""
    seen["tests"].add(request.node.originalname)

    @contextlib.contextmanager
    def use(poison, lib=None, ws_word=None):
        real = lib if lib is not None else eng._lib()
        dev = eng._device(None)
        proxy = ContractProxy(real, Memory(dev, real), poison=poison, ws_word=ws_word, record=seen["calls"])
        with monkeypatch.context() as m:
            m.setattr(_native, "_LIB", proxy)
            yield proxy
    return use


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _tuple(r):
    """The results of a call by their positions: a single array is (array,), an output not asked for stays None."""
    return tuple(r) if isinstance(r, (tuple, list)) else (r,)


def check_case(poisoned, run, want=None):
    """run() on the caller's buffers and under the three poisons: the same bits every time, and those of `want`, position
    by position (an array for a single result; None at a position: no exact reference here, or no such output).  Returns
    the results of the plain run by position."""
    plain = _tuple(run())
    for poison in POISONS:
        with poisoned(poison) as proxy:
            got = _tuple(run())
        assert sum(proxy.called.values()) >= 1, "the case did not reach the library"
        assert len(got) == len(plain)
        for k, (g, p) in enumerate(zip(got, plain)):
            assert (g is None) == (p is None), k
            assert g is None or same_bits(g, p), f"poison {poison:#04x}: result {k} differs from the run on the caller's buffers"
    if want is not None:
        want = _tuple(want)
        assert len(want) == len(plain), "one reference (or None) per result"
        for k, w in enumerate(want):
            if w is not None:
                assert plain[k] is not None, k
                assert np.array_equal(np.asarray(plain[k]), np.asarray(w), equal_nan=np.asarray(w).dtype.kind == "f"), \
                    f"result {k} differs from the reference"
    return plain


# ---------------------------------------------------------------------------------------------------- data
@functools.lru_cache(maxsize=None)
def curves(T, n, seed=0, nan=True, ties=True):
    """T x n: random walks rounded to one decimal (ties), one NaN column entry and one infinite row where asked."""
    rng = np.random.default_rng([seed, T, n])
    X = rng.normal(size=(T, n)).cumsum(axis=0)
    if ties:
        X = np.round(X, 1)
    if nan:
        X[T // 2, n // 3] = np.nan
        X[T - 1, n // 2] = np.inf
    X.setflags(write=False)
    return X


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def blocks_of(n, nb, bs, seed):
    """nb blocks of up to bs distinct rows, -1 padded at the end, the target last."""
    rng = np.random.default_rng(seed)
    mem = np.full((nb, bs), -1, dtype=np.int32)
    for k in range(nb):
        size = int(rng.integers(max(2, bs // 2), bs + 1))
        mem[k, :size] = rng.choice(n, size=size, replace=False)
    return mem


def block_rows(mem):
    return [row[row >= 0] for row in mem]


# ---------------------------------------------------------------------------------------------------- K1 + K2
MBD_ROUTES = [
    # id, T, n, J, algo, targets
    ("pairwise", 12, 70, 3, "pairwise", None),
    ("pairwise-targets", 12, 70, 2, "pairwise", [5, 0, 69, 5]),
    ("bucket-fold-J2", 40, 300, 2, "rank", None),
    ("bucket-fold-J3-targets", 40, 1025, 3, "rank", [7, 1024, 0]),
    ("pair-image-J4", 9, 65, 4, "rank", None),
    ("auto", 40, 300, 2, "auto", None),
]


@pytest.mark.parametrize("name,T,n,J,algo,targets", MBD_ROUTES, ids=[r[0] for r in MBD_ROUTES])
def test_mbd_counts_small_routes(eng, oracle, poisoned, name, T, n, J, algo, targets):
    X = curves(T, n)
    check_case(poisoned, lambda: eng.mbd_counts(X, targets, J, algo=algo), oracle.mbd_counts(X, targets, J))


def test_mbd_two_launch_path(eng, oracle, poisoned):
    """Just above the path's lower bound on n, rows > 2 x CUs so that some workgroups rank two rows; tie-heavy rows, a NaN
    and an infinity: flagged rows for the second launch.  Then a target subset: the totals of all curves in the workspace."""
    T, n = 2 * cus() + 8, 3073
    X = curves(T, n)
    want = oracle.mbd_counts_ranksort(X, 2)
    check_case(poisoned, lambda: eng.mbd_counts(X, None, 2, algo="rank"), want)
    tg = np.array([3072, 0, 17, 17])
    check_case(poisoned, lambda: eng.mbd_counts(X, tg, 2, algo="rank"), want[tg])
    Y = curves(T, n, nan=False, ties=False)                          # continuous: nothing flagged, the second launch returns early
    check_case(poisoned, lambda: eng.mbd_counts(Y, None, 2, algo="rank"), oracle.mbd_counts_ranksort(Y, 2))


def test_mbd_medium_image_route(eng, oracle, poisoned):
    X = curves(96, 16385)
    check_case(poisoned, lambda: eng.mbd_counts(X, None, 2, algo="rank"), oracle.mbd_counts_ranksort(X, 2))


def test_mbd_large_n_route(eng, oracle, poisoned):
    X = curves(2, 16385)
    check_case(poisoned, lambda: eng.mbd_counts(X, None, 2, algo="rank"), oracle.mbd_counts_ranksort(X, 2))
    check_case(poisoned, lambda: eng.mbd_counts(X, [16384, 3], 3, algo="rank"), oracle.mbd_counts(X, [16384, 3], 3))


def test_mbd_range_wide_external_subset_above_below(eng, oracle, poisoned):
    X = curves(23, 90)
    full = oracle.mbd_counts(X, None, 3)
    check_case(poisoned, lambda: eng.mbd_counts_range(X, 31, 40, 3, algo="rank"), full[31:71])
    check_case(poisoned, lambda: eng.mbd_counts_range(np.asfortranarray(X), 31, 40, 3, algo="pairwise"), full[31:71])
    wide = check_case(poisoned, lambda: eng.mbd_counts_wide(X, [4, 89], 3, algo="rank").astype(np.float64))[0]
    assert np.array_equal(wide, full[[4, 89]].astype(np.float64))
    Q = np.ascontiguousarray(X[:, [3, 30, 30]] + 0.05)
    want = np.stack([oracle.mbd_counts(np.column_stack([X, Q[:, q]]), [90], 3)[0] for q in range(3)])
    check_case(poisoned, lambda: eng.mbd_external_counts(X, Q, 3), want)
    mem = blocks_of(90, 12, 33, 1)
    tg = np.array([row[-1] for row in block_rows(mem)], dtype=np.int32)
    want = np.stack([oracle.mbd_counts(X[:, row], [len(row) - 1], 3)[0] for row in block_rows(mem)])
    check_case(poisoned, lambda: eng.mbd_subset_counts(X, mem, tg, 3), want)
    check_case(poisoned, lambda: eng.above_below(X, [0, 89, 44]), oracle.above_below(X, [0, 89, 44]))


# ---------------------------------------------------------------------------------------------------- K3
STRICT_ROUTES = [
    # id, T, n, NaN, J, budget
    ("classes-T3", 3, 200, False, 2, None),
    ("classes-T4-nan", 4, 200, True, 2, None),
    ("class-wg-T7", 7, 300, False, 2, None),
    ("masks-T7-nan", 7, 300, True, 2, None),
    ("match-T20", 20, 300, True, 2, None),
    ("match-T20-floor", 20, 300, True, 2, 1),
    ("match-T70-floor", 70, 130, True, 2, 1),
    ("subsets-J3", 10, 40, True, 3, None),
    ("subsets-J3-floor", 10, 40, True, 3, 1),
]


@pytest.mark.parametrize("name,T,n,nan,J,budget", STRICT_ROUTES, ids=[r[0] for r in STRICT_ROUTES])
def test_strict_routes(eng, oracle, poisoned, name, T, n, nan, J, budget):
    X = curves(T, n, nan=nan)
    want = oracle.bd_strict_counts(X)[:, None] if J == 2 else oracle.band_enum(X, None, J, relax=False)
    check_case(poisoned, lambda: eng.bd_strict_counts(X, None, J, workspace_budget=budget), want)
    tg = [n - 1, 0, 5]
    check_case(poisoned, lambda: eng.bd_strict_counts(X, tg, J, workspace_budget=budget), want[tg])


def test_strict_grid_and_rank32(eng, oracle, poisoned):
    """The two routes of large n at their smallest shapes, recommended size and floor, sampled targets against the
    oracle's class counting.  Grid of cells: n = 32 768, T = 3, every curve a target, then every fourth (the subset plan);
    at the floor the grid has no room and the state-class kernel takes the call.  32-bit rank image: n = 32 768, T = 8 with
    a NaN (the classes of 6 to 8 timepoints step aside), four targets; the large-n route's scratch with its gate words lies
    inside this workspace."""
    n = 32768
    X = curves(3, n, nan=False)                                      # rounded: every value repeats
    sample = np.arange(0, n, 2731)
    want = oracle.bd_strict_counts_by_states(X, sample)
    every4 = np.arange(0, n, 4)
    for budget in (None, 1):
        got = check_case(poisoned, lambda: eng.bd_strict_counts(X, None, 2, workspace_budget=budget))[0]
        assert np.array_equal(got[sample, 0], want)
        part = check_case(poisoned, lambda: eng.bd_strict_counts(X, every4, 2, workspace_budget=budget))[0]
        assert np.array_equal(part[:, 0], got[every4, 0])
    Z = curves(8, n)
    tg = np.array([0, n - 1, 5, n // 3])                             # the last one is the curve with the NaN
    want = oracle.bd_strict_counts_by_states(Z, tg)
    assert want[3] == 0 and want[:3].min() > 0
    for budget in (None, 1):
        check_case(poisoned, lambda: eng.bd_strict_counts(Z, tg, 2, workspace_budget=budget), want[:, None])


def test_strict_j2_entry_point_external_and_subset(eng, oracle, poisoned):
    """sd_bd_strict_counts has no engine wrapper: through the ABI with tensors of the test's own."""
    import torch
    T, n = 20, 150
    X = curves(T, n)
    want = oracle.bd_strict_counts(X)

    def direct():
        lib = _native.load()
        dev = eng._device(None)
        Xd = torch.from_numpy(np.ascontiguousarray(X)).to(dev)
        out = torch.empty(n, dtype=torch.int64, device=dev)
        size = int(lib.sd_bd_strict_workspace_bytes(T, n, n, 1, n))
        ws = torch.empty(size, dtype=torch.uint8, device=dev)
        _native.check(lib.sd_bd_strict_counts(Xd.data_ptr(), T, n, n, 1, None, n, out.data_ptr(), ws.data_ptr(), size,
                                              torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize(dev)
        return out.cpu().numpy()
    check_case(poisoned, direct, want)
    Q = np.ascontiguousarray(X[:, [3, 30]] + 0.05)
    want = np.array([oracle.bd_strict_counts(np.column_stack([X, Q[:, q]]), [n])[0] for q in range(2)])
    check_case(poisoned, lambda: eng.bd_strict_external_counts(X, Q), want)
    for bs in (33, 140):                                             # masks in LDS, then in the workspace
        Z = curves(300 if bs > 100 else T, n)
        mem = blocks_of(n, 10, bs, bs)
        rows = block_rows(mem)
        tg = np.array([row[-1] for row in rows], dtype=np.int32)
        want = np.array([oracle.bd_strict_counts(Z[:, row], [len(row) - 1])[0] for row in rows])
        check_case(poisoned, lambda: eng.bd_strict_subset_counts(Z, mem, tg), want)


# ---------------------------------------------------------------------------------------------------- point clouds
def cloud(n, d, seed=0):
    P = np.round(np.random.default_rng([seed, n, d]).normal(size=(n, d)), 2)
    P[n // 2] = P[0]                                                  # a duplicate
    return P


def test_l1_oja_simplex_forms(eng, oracle, poisoned):
    P, Q = cloud(70, 3), cloud(5, 3, 1)
    mem = blocks_of(70, 6, 20, 2)
    tg = [69, 0, 35]
    L = np.random.default_rng(4).normal(size=(70, 3))                # L1: no coincident points (0 / 0 is NaN by contract)

    def l1_check(got, ref, sizes):
        err = l1_errors(got, ref)
        assert np.all(err <= np.array([l1_tolerance(N, 3) for N in sizes])), err
    l1_check(check_case(poisoned, lambda: eng.l1_depth(L, tg))[0], l1_reference(L, tg), [70] * 3)
    l1_check(check_case(poisoned, lambda: eng.l1_external_depth(L, Q))[0], l1_reference(L, Q=Q), [71] * len(Q))
    l1_check(check_case(poisoned, lambda: eng.l1_subset_depth(L, mem))[0], l1_reference(L, blocks=mem),
             [len(r) for r in block_rows(mem)])
    # the Oja module's criterion: assert_depths_close at 1e-12 against the determinant sums of the definition
    assert_depths_close(check_case(poisoned, lambda: eng.oja_volume_sums(P, tg))[0], oja_sums(P, tg), 1e-12)
    assert_depths_close(check_case(poisoned, lambda: eng.oja_external_volume_sums(P, Q))[0],
                        np.array([oja_sums(np.vstack([P, q]), [len(P)])[0] for q in Q]), 1e-12)
    assert_depths_close(check_case(poisoned, lambda: eng.oja_subset_volume_sums(P, mem))[0],
                        np.array([oja_sums(P[r], [len(r) - 1])[0] for r in block_rows(mem)]), 1e-12)
    S = cloud(24, 2)
    check_case(poisoned, lambda: eng.pointcloud_simplex_counts(S, [0, 23, 7]), oracle.pointcloud_simplex_counts(S, [0, 23, 7]))
    want = np.array([oracle.pointcloud_simplex_counts(np.vstack([S, q]), [24])[0] for q in Q[:, :2]])
    check_case(poisoned, lambda: eng.pointcloud_simplex_external_counts(S, Q[:, :2]), want)
    smem = blocks_of(24, 5, 12, 3)
    want = np.array([oracle.pointcloud_simplex_counts(S[row], [len(row) - 1])[0] for row in block_rows(smem)])
    check_case(poisoned, lambda: eng.pointcloud_simplex_subset_counts(S, smem), want)
    # the sampled estimators: the recommended workspace (two kernels), none at all (one kernel) and a third of it
    rec = int(eng._lib().sd_simplex_sampled_workspace_bytes(70, 0, 3, 64))
    for ws in (None, 0, rec // 3):
        check_case(poisoned, lambda: eng.pointcloud_simplex_counts(P, tg, samples=64, seed=3, ws_bytes=ws),
                   oracle.simplex_sampled(P, tg, samples=64, seed=3))
    M = np.round(np.random.default_rng(5).normal(size=(14, 4, 2)), 1)
    for relax in (True, False):
        check_case(poisoned, lambda: eng.multi_simplex_counts(M, [0, 13], relax), oracle.multi_simplex_counts(M, [0, 13], relax))
    rec = int(eng._lib().sd_simplex_sampled_workspace_bytes(14, 4, 2, 32))
    for ws in (None, 0, rec // 3):
        check_case(poisoned, lambda: eng.multi_simplex_counts(M, None, True, samples=32, seed=1, ws_bytes=ws),
                   oracle.simplex_sampled(M, None, True, samples=32, seed=1))


def test_multi_band(eng, oracle, poisoned):
    P = np.round(np.random.default_rng(6).normal(size=(40, 9, 2)).cumsum(axis=1), 1)
    check_case(poisoned, lambda: eng.multi_band_counts(P, [0, 39, 7]), oracle.multi_band_enum(P, [0, 39, 7], 2)[:, 0])
    for J in (2, 3, 4):
        check_case(poisoned, lambda: eng.multi_band_j_counts(P[:24], None, J), oracle.multi_band_enum(P[:24], None, J))


def test_probabilistic_sums(eng, poisoned):
    rng = np.random.default_rng(7)
    mu, sigma = rng.normal(size=60), rng.uniform(0.1, 2.0, size=60)
    def rel_close(got, want, rtol):
        assert np.isfinite(got).all() and np.all(np.abs(got - want) <= rtol * np.abs(want) + 1e-300), (got, want)
    c = math.comb(60, 2)                                             # the criteria of the three families' own modules
    got = check_case(poisoned, lambda: eng.prob_normal_sums(mu, sigma, [0, 59, 3]))[0]
    assert np.max(np.abs(got / c - normal_sums(mu, sigma, [0, 59, 3]) / c)) <= 1e-12
    lam = rng.uniform(0.5, 9.0, size=(5, 30))
    rel_close(check_case(poisoned, lambda: eng.prob_poisson_sums(lam, 25, [0, 29]))[0], poisson_sums(lam, 25, [0, 29]), 1e-12)
    m2, v2 = rng.normal(size=(6, 40)), rng.uniform(0.0, 1.0, size=(6, 40))
    v2[:, 3] = 0.0                                                    # a point mass
    for relax, rtol in ((True, 1e-13), (False, 1e-10)):
        rel_close(check_case(poisoned, lambda: eng.prob_band_sums(m2, v2, relax, [0, 39, 3]))[0],
                  band_sums(m2, v2, relax, [0, 39, 3]), rtol)
    mem = blocks_of(40, 3, 15, 8)
    rel_close(check_case(poisoned, lambda: eng.prob_band_sums(m2, v2, True, [0, 39, 3], members=mem))[0],
              band_sums(m2, v2, True, [0, 39, 3], members=mem), 1e-13)


def test_halfspace_and_projection_forms(eng, poisoned):
    n, d, k = 2049, 3, 9                                             # the sort across one full network and a key
    P, Q = cloud(n, d), cloud(4, d, 1)
    U = make_directions(k, 11, d)
    tg = [0, n - 1, n // 2]
    mem = blocks_of(n, 6, 40, 9)
    rows = block_rows(mem)
    H = halfspace_counts_sorted(P, U)
    check_case(poisoned, lambda: eng.halfspace_counts(P, U), H)
    check_case(poisoned, lambda: eng.halfspace_counts(P, U, tg, workspace_budget=0), H[tg])       # the floor: one direction a chunk
    check_case(poisoned, lambda: eng.halfspace_counts(P, U, tg, algo="pairwise"), H[tg])
    check_case(poisoned, lambda: eng.halfspace_external_counts(P, Q, U), halfspace_external(P, Q, U))
    check_case(poisoned, lambda: eng.halfspace_subset_counts(P, mem, U),
               np.array([halfspace_counts_sorted(P[r], U, [len(r) - 1])[0] for r in rows]))
    O = projection_outlyingness(P, U)
    check_case(poisoned, lambda: eng.projection_outlyingness(P, U), O)
    check_case(poisoned, lambda: eng.projection_outlyingness(P, U, tg, workspace_budget=0), O[tg])
    check_case(poisoned, lambda: eng.projection_external_outlyingness(P, Q, U), projection_external(P, Q, U))
    check_case(poisoned, lambda: eng.projection_external_outlyingness(P, Q, U, workspace_budget=0), projection_external(P, Q, U))
    check_case(poisoned, lambda: eng.projection_subset_outlyingness(P, mem, U),
               np.array([projection_outlyingness(P[r], U, [len(r) - 1])[0] for r in rows]))


@pytest.mark.parametrize("algo", ["sweep", "pairwise"])
def test_exact_planar_forms(eng, poisoned, algo):
    P, Q = integer_cloud(130, 3), integer_cloud(5, 4) + 0.5
    mem = blocks_of(130, 6, 30, 10)
    rows = block_rows(mem)
    tg = [0, 129, 64]
    check_case(poisoned, lambda: eng.halfspace_exact_counts(P, tg, algo=algo), exact_counts(P, tg))
    check_case(poisoned, lambda: eng.halfspace_exact_external_counts(P, Q, algo=algo), exact_external(P, Q))
    check_case(poisoned, lambda: eng.halfspace_exact_subset_counts(P, mem, algo=algo),
               np.array([exact_counts(P[r], [len(r) - 1])[0] for r in rows]))
    check_case(poisoned, lambda: eng.simplicial_exact_counts(P, tg, algo=algo), simplicial_counts(P, tg))
    check_case(poisoned, lambda: eng.simplicial_exact_external_counts(P, Q, algo=algo), simplicial_external(P, Q))
    check_case(poisoned, lambda: eng.simplicial_exact_subset_counts(P, mem, algo=algo),
               np.array([simplicial_counts(P[r], [len(r) - 1])[0] for r in rows]))


# ---------------------------------------------------------------------------------------------------- curves on the pair image
@pytest.mark.parametrize("algo", ["image", "sort"])
@pytest.mark.parametrize("curve_major", [False, True])
def test_rank_depths_extremal_tvd(eng, poisoned, algo, curve_major):
    """T = 19 rows: at the floor one row a batch, so every slice record, the carried row and the extremity matrix cross
    18 batch boundaries."""
    T, n = 19, 65
    X = curves(T, n, nan=False)
    M = np.asfortranarray(X) if curve_major else X
    tg = np.array([64, 0, 7, 7])
    rec = records_np(X)
    ext = extremal_counts_lexsort(X)
    a, c = tvd_counts_np(X)
    sd = (a * (n - a)).sum(axis=0)
    tv = {"image": "lds", "sort": "pairwise"}[algo]
    for floor in (False, True):
        ws = [fn(T, n, algo=al, curve_major=curve_major)[1] if floor else None
              for fn, al in ((eng.rank_depth_workspace_bytes, algo), (eng.extremal_workspace_bytes, algo))]
        tws = eng.tvd_workspace_bytes(T, n, algo=tv, curve_major=curve_major, m=len(tg))[1] if floor else None
        check_case(poisoned, lambda: eng.rank_depth_sums(M, tg, algo=algo, ws_bytes=ws[0]), rec[tg])
        check_case(poisoned, lambda: eng.extremal_counts(M, tg, algo=algo, ws_bytes=ws[1]), ext[tg])
        shape = check_case(poisoned, lambda: eng.tvd_sums(M, tg, algo=tv, ws_bytes=tws, counts=True), (sd[tg], None, c[:, tg]))[1]
        check_doubles(X, shape, tg, T)
    check_case(poisoned, lambda: eng.tvd_sums(M, None, algo=tv), (sd, None))


def test_sort_route_above_one_network(eng, poisoned):
    X = curves(3, 2049, nan=False)
    check_case(poisoned, lambda: eng.rank_depth_sums(X, algo="sort"), records_np(X))
    check_case(poisoned, lambda: eng.extremal_counts(X, [0, 2048], algo="sort"), extremal_counts_lexsort(X)[[0, 2048]])


@pytest.mark.parametrize("curve_major", [False, True])
def test_central_regions(eng, poisoned, curve_major):
    cap = eng.central_regions_row_capacity()
    for n in (65, cap + 1):                                          # rows in one workgroup's registers, then column blocks
        X = curves(5, n, nan=False)
        M = np.asfortranarray(X) if curve_major else X
        level = (np.arange(n) % 4).astype(np.uint8)
        check_case(poisoned, lambda: eng.central_regions(M, level, 3, box=1), boxplot_np(X, level, 3, box=1, factor=1.5))
        check_case(poisoned, lambda: eng.central_regions(M, level, 3), boxplot_np(X, level, 3))
        env, _, _, whisker = boxplot_np(X, level, 3, box=0, factor=1.5)
        check_case(poisoned, lambda: eng.central_regions(M, level, 3, box=0, outside=False, fence=False),
                   (env, None, None, whisker))


# ---------------------------------------------------------------------------------------------------- multivariate curves over time
@pytest.mark.parametrize("algo", ["lds", "global"])
def test_multi_cloud_families(eng, poisoned, algo):
    n, T, d, k = 100, 5, 3, 40
    P = np.random.default_rng(12).normal(size=(n, T, d))
    U = make_directions(k, 13, d)
    tg = [99, 0, 3]
    H, O = multi_halfspace_records(P, U), multi_projection_records(P, U)
    rec, cen, cur = multi_outlyingness_records(P, U, centres=True, curves=True)
    for floor in (False, True):
        ws = [fn(n, T, d, k, len(tg), algo)[1] if floor else None for fn in
              (eng.multi_halfspace_workspace_bytes, eng.multi_projection_workspace_bytes, eng.multi_outlyingness_workspace_bytes)]
        check_case(poisoned, lambda: eng.multi_halfspace_sums(P, U, tg, algo=algo, ws_bytes=ws[0]), H[tg])
        check_case(poisoned, lambda: eng.multi_projection_sums(P, U, tg, algo=algo, ws_bytes=ws[1]), O[tg])
        check_case(poisoned, lambda: eng.multi_outlyingness_moments(P, U, tg, algo=algo, ws_bytes=ws[2], centres=True, curves=True),
                   (rec[tg], cen, cur[tg]))
    check_case(poisoned, lambda: eng.multi_outlyingness_moments(P, U, None, algo=algo), rec)


# ---------------------------------------------------------------------------------------------------- the metric depths
KAPPAS = (0.0, 1.0, 0.25)
SPATIAL_EXACT = 24                                                   # targets whose S and E are restated in exact arithmetic


@functools.lru_cache(maxsize=None)
def metric_case():
    """(X, Q, targets, D2, DQ, lens counts of the first 40 targets and of Q per kappa), computed once and not modified."""
    T, n = 5, 257
    X = curves(T, n, nan=False)
    Q = np.ascontiguousarray(X[:, ::2] + 0.25)                       # 129 external targets: two blocks
    tg = np.arange(n)[::-1].copy()
    D2 = sqdist_exact(X)
    DQ = sqdist_exact(np.concatenate([X, Q], axis=1), n + np.arange(Q.shape[1]))[:, :n]
    lens = {kappa: (lens_counts_np(D2, D2[tg[:40]], kappa), lens_counts_np(D2, DQ, kappa)) for kappa in KAPPAS}
    spatial = spatial_exact(X, tg[:SPATIAL_EXACT]) + spatial_exact(X, Q=Q[:, :SPATIAL_EXACT])
    return X, Q, tg, D2, DQ, lens, spatial


@pytest.mark.parametrize("curve_major", [False, True])
def test_metric_depths(eng, poisoned, curve_major):
    """n = 257: three blocks of 128 targets, so the floor (one block a batch) walks three batches."""
    X, Q, tg, D2, DQ, lens, (S, E, SQ, EQ) = metric_case()
    ke = SPATIAL_EXACT
    T, n = X.shape
    M = np.asfortranarray(X) if curve_major else X
    sizes = lambda fn, **kw: fn(T, n, curve_major=curve_major, **kw)
    check_case(poisoned, lambda: eng.curve_sqdist(M, tg), D2[tg])
    check_case(poisoned, lambda: eng.curve_sqdist_external(X, Q), DQ)
    pairs = np.sort(D2[np.triu_indices(n, 1)])
    for what in ("recommended", "floor"):
        pick = 0 if what == "recommended" else 1
        ws = sizes(eng.curve_sqdist_workspace_bytes, what="select")[pick]
        k = len(pairs) // 3
        got = check_case(poisoned, lambda: np.array([eng.curve_sqdist_select(M, k, ws_bytes=ws)]))[0]
        assert got[0] == pairs[k - 1]
        ws = sizes(eng.curve_sqdist_workspace_bytes, what="hmodal")[pick]
        check_sums(check_case(poisoned, lambda: eng.hmodal_sums(M, 0.01, tg, ws_bytes=ws))[0][:32], D2[tg[:32]], 0.01, n)
        ws = eng.curve_sqdist_workspace_bytes(T, n, what="hmodal", m=Q.shape[1])[pick]
        check_sums(check_case(poisoned, lambda: eng.hmodal_external_sums(X, Q, 0.01, ws_bytes=ws))[0][:32], DQ[:32], 0.01, n)
        ws = sizes(eng.spatial_workspace_bytes)[pick]
        got = check_case(poisoned, lambda: eng.spatial_sums(M, tg, ws_bytes=ws, field=True))    # the spatial module's criterion:
        assert np.array_equal(got[0][:ke], S) and np.array_equal(got[1][:ke], E)                  # the restatement's values
        got = check_case(poisoned, lambda: eng.spatial_sums(M, None, ws_bytes=ws))
        assert np.array_equal(got[0][tg[:ke]], S)
        ws = eng.spatial_workspace_bytes(T, n, m=Q.shape[1])[pick]
        got = check_case(poisoned, lambda: eng.spatial_external_sums(X, Q, ws_bytes=ws, field=True))
        assert np.array_equal(got[0][:ke], SQ) and np.array_equal(got[1][:ke], EQ)
        for kappa in KAPPAS:
            ws = sizes(eng.lens_workspace_bytes)[pick]
            check_case(poisoned, lambda: eng.lens_counts(M, kappa, tg[:40], ws_bytes=ws), lens[kappa][0])
            ws = eng.lens_workspace_bytes(T, n, m=Q.shape[1])[pick]
            check_case(poisoned, lambda: eng.lens_external_counts(X, Q, kappa, ws_bytes=ws), lens[kappa][1])


# ---------------------------------------------------------------------------------------------------- stale gate words
def fresh_library(eng, tmp_path, source, tag):
    """A second instance of the library with statics of its own: its epoch counters start at 0.  (The engine's device
    first: torch has to find the device before a library starts the HIP runtime.)"""
    eng._device(None)
    path = tmp_path / f"{tag}.so"
    shutil.copyfile(source, path)
    return _native.open_library(str(path))


def eight_calls(eng, poisoned, lib, word, X, want):
    """Eight consecutive calls (epochs 1 .. 8 of a fresh library, one batch each) on workspaces full of `word`."""
    for call in range(8):
        with poisoned(0xA5, lib=lib, ws_word=word) as proxy:
            got = eng.mbd_counts(X, None, 2, algo="rank")
        assert proxy.guarded_workspaces["sd_mbd_counts"] == 1
        assert np.array_equal(got, want), f"call {call + 1} (epoch {call + 1}) on a workspace full of {word:#x}"


@pytest.mark.parametrize("word", [4, 4 << 8 | 0xFF, 4 << 8 | 5], ids=["gate0", "gate1", "gate1-count5"])
@pytest.mark.parametrize("data", ["continuous", "flagged"])
def test_stale_gate_words_of_the_two_launch_path(eng, oracle, poisoned, tmp_path, word, data):
    """The smallest n of the path, every curve a target, 2 x CUs + 8 rows (a workgroup reads gate[1] in front of its second
    row only).  The fourth call finds gate[0] "set" (word 4), or gate[1] saying "epoch 4, 255 contenders: stop", or "epoch 4,
    five contenders", which the genuine contenders of the flagged data count on from."""
    T, n = 2 * cus() + 8, 3073
    if data == "continuous":
        X = curves(T, n, nan=False, ties=False)
    else:
        X = np.array(curves(T, n, nan=False, ties=False))
        X[3] = np.round(X[3], 0)                                     # tie-heavy rows and a NaN row among the first workgroups' rows
        X[5] = np.round(X[5], 0)
        X[9, ::7] = np.nan
        X[T - 2] = 1.0
    want = oracle.mbd_counts_ranksort(X, 2)
    eight_calls(eng, poisoned, fresh_library(eng, tmp_path, _native.LIB_PATH, "two_launch"), word, X, want)


@pytest.mark.parametrize("data", ["continuous", "flagged"])
def test_stale_gate_words_of_the_large_n_route(eng, oracle, poisoned, tmp_path, monkeypatch, data):
    """n = 16 385, T = 2: one batch a call, the word 4 in gate[0] and gate[1] alike.  Then one call of three batches on a
    fresh copy of the cross-check library (one row a batch): the epoch advances inside the call, past the word."""
    n = 16385
    X = np.array(curves(3, n, nan=False, ties=False))
    if data == "flagged":
        X[1] = np.round(X[1], 0)                                     # tie-heavy: flagged value buckets
        X[0, ::5] = np.nan
        X[2, :9000] = 2.5                                            # more equal keys than a value bucket holds
    eight_calls(eng, poisoned, fresh_library(eng, tmp_path, _native.LIB_PATH, "large_n"), 4, X[:2], oracle.mbd_counts_ranksort(X[:2], 2))
    monkeypatch.setenv("SD_RANK_ROWS_PER_BATCH", "1")
    want = oracle.mbd_counts_ranksort(X, 2)
    for word in (2, 3):                                               # the second and the third batch of a library's first call
        lib = fresh_library(eng, tmp_path, _native.XCHECK_LIB_PATH, f"large_n_batches_{word}")
        assert lib.sd_is_crosscheck_build() == 1
        with poisoned(0xA5, lib=lib, ws_word=word):
            assert np.array_equal(eng.mbd_counts(X, None, 2, algo="rank"), want), word


# ---------------------------------------------------------------------------------------------------- coverage
def test_every_entry_point_was_exercised_under_every_poison(seen):
    """Asserted when every test function of the module ran in this process (a selection by -k or a worker's share of the
    module cannot have seen everything, and says nothing about the table)."""
    cases = {name for name, obj in globals().items() if name.startswith("test_") and callable(obj)}
    cases.discard("test_every_entry_point_was_exercised_under_every_poison")
    if cases - seen["tests"]:
        print("coverage not asserted, these cases did not run here:", sorted(cases - seen["tests"]))
        return
    missing = [(name, hex(p)) for name in compute_symbols() for p in POISONS if (name, p) not in seen["calls"]]
    assert not missing, missing
    assert set(OUTPUTS) == {name for name, _ in seen["calls"]}
