/*
 * statdepth_hip.h -- C ABI of the MI355X (gfx950) band-depth engine.
 *
 * This is the drop-in boundary for statdepth's calculation layer
 * (the files under statdepth/depth/calculations/ in the reference).  The reference has no
 * FFI of its own -- its hot path is Python loops -- so each entry point below
 * names the reference function whose inner loops it replaces; the host side
 * (statdepth_amd/, Python) keeps the reference's FunctionalDepth /
 * PointcloudDepth signatures and calls these through ctypes.  INTEGRATION.md
 * shows the stub a statdepth maintainer would add to bind them.
 *
 * Conventions
 *  - plain C types only; every data pointer is a DEVICE pointer (HBM) unless
 *    the name says host; `stream` is a hipStream_t passed as void* (NULL = the
 *    null stream).  Calls enqueue work and return; they do not synchronise.
 *  - a univariate data set of n curves observed at T timepoints is addressed
 *    as x(t,i) = X[t*st + i*sn] (strides in elements), so both pandas layouts
 *    are accepted in place: C-contiguous T x n ("time-major", st=n, sn=1) and
 *    F-contiguous ("curve-major", st=1, sn=T).  Kernels run time-major; a
 *    curve-major input is transposed on the device into the workspace first.
 *  - `targets` is an int64 device array of m curve / point indices (the
 *    reference's `to_compute`), or NULL for "all, in order" (then m must be n).
 *  - integer outputs are the tested contract (bit-exact vs the reference);
 *    the fp64 normalisers (/T, /C(n,j) ...) stay on the host.
 *  - every function returns SD_OK (0) or an error code; sd_last_error() gives
 *    the message for the calling thread.
 *
 * Caller memory: the workspace and the outputs
 * Every sd_* call that takes `ws` / `ws_bytes` or an output pointer keeps to this:
 *  - `ws` may hold ANY bytes on entry.  Whatever a call reads from its
 *    workspace, a launch of the same call has written before -- counters,
 *    flags, slice records, carried rows and the words indices are read from
 *    included.  The two rank routes whose gate words are never zeroed
 *    (mbd_rank_bucket.hip, mbd_rank_big.hip: a word is "set" when it equals
 *    the call's epoch) give the same results when a stale word happens to
 *    equal the epoch; it costs time only.
 *  - nothing in `ws` is needed after the call's work has run: the next call
 *    on the stream may get the same buffer, or any other.  The library keeps
 *    no pointer into it.
 *  - the caller passes `ws` 256-byte aligned.
 *  - no byte is written outside [ws, ws + ws_bytes), whatever ws_bytes is --
 *    the recommended size, the floor of a family that has one, or anything
 *    between; below what a call needs it returns SD_ERR_WORKSPACE.
 *  - no byte is written outside the documented extent of an output (m int64,
 *    m x (J - 1) int64, ... as each entry point states; nothing is rounded up
 *    to a tile or a vector).
 *  - outputs may hold ANY bytes on entry: a call that adds into an output or
 *    takes minima on it initialises it on its own stream first.  No entry
 *    point asks the caller to zero anything -- sd_mbd_counts_wide, and the
 *    `centres` and `curves` of sd_multi_outlyingness_moments, store every
 *    element they document.
 *  - calls enqueue and return, with one documented exception: the strict
 *    band depth (sd_bd_strict_counts, sd_bd_strict_j_counts,
 *    sd_bd_strict_external_counts) of series of 6 to 8 timepoints at J = 2
 *    waits for the stream once, in the middle of the call: a NaN flag comes
 *    back to the host and decides between two routes.
 * tests/workspace_contract.py enforces these at this boundary: guard bands
 * around a workspace of exactly ws_bytes and around every output, three
 * poison patterns in both, for every entry point and route.
 */
#ifndef STATDEPTH_HIP_H
#define STATDEPTH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SD_ABI_VERSION 1

enum sd_status {
    SD_OK = 0,
    SD_ERR_INVALID = 1,     /* bad argument (shape, stride, J, null pointer ...) */
    SD_ERR_HIP = 2,         /* a HIP runtime call failed */
    SD_ERR_NO_DEVICE = 3,   /* no gfx950 device visible */
    SD_ERR_UNSUPPORTED = 4, /* valid request outside what the kernels cover */
    SD_ERR_OVERFLOW = 5,    /* an int64 total could overflow (T*C(n-1,J) >= 2^63) */
    SD_ERR_WORKSPACE = 6    /* workspace too small */
};

/* algorithm selector of sd_mbd_counts */
enum sd_mbd_algo {
    SD_MBD_AUTO = 0,
    SD_MBD_PAIRWISE = 1, /* O(m n T): stream every curve against every target, compare + count */
    SD_MBD_RANK = 2      /* O(n T log n): per-timepoint sort in LDS, ranks give the same integers */
};

/* ---- library / device ---------------------------------------------------- */
int sd_abi_version(void);
/* 0 for the product library.  1 for libstatdepth_hip_xcheck.so, which links the same objects and
 * also holds the retired kernel generations and honours the SD_* environment switches selecting them (tests only). */
int sd_is_crosscheck_build(void);
const char *sd_last_error(void);
int sd_device_count(void);
/* name (e.g. "gfx950...") and CU count of device `dev`; name buffer >= 64 bytes */
int sd_device_info(int dev, char *name, int name_len, int *cu_count, size_t *hbm_bytes);
int sd_set_device(int dev);

/* ---- memory / stream helpers for clients without their own allocator ------ */
int sd_malloc(void **dptr, size_t bytes);
int sd_free(void *dptr);
int sd_memcpy_h2d(void *dst, const void *src_host, size_t bytes, void *stream);
int sd_memcpy_d2h(void *dst_host, const void *src, size_t bytes, void *stream);
int sd_memset(void *dst, int value, size_t bytes, void *stream);
int sd_stream_synchronize(void *stream);

/* ---- K1+K2: modified band depth totals (relax=True) ------------------------
 * Replaces: the subset loop of _univariate_band_depth (_functional.py:238-253)
 * with _r2_containment(relax=True) (_containment.py:45-80) inside it, for all
 * targets of _functionaldepth's loop (_functional.py:74-75).
 *
 * out[q*(J-1) + (j-2)] = sum over t of #{j-subsets of the OTHER n-1 curves whose
 * band [min,max] (pandas skipna, inclusive ends) contains target q at t},
 * j = 2..J.  The host forms S_nj = out/T and depth = sum_j S_nj / C(n,j).
 * Computed from per-timepoint counts A (others strictly above), B (strictly
 * below), N (NaN others), v = n-1-N:
 *     sum_{k=1..j} C(N,j-k) * [C(v,k) - C(A,k) - C(B,k)]       (0 if x is NaN)
 * which equals the reference's enumeration exactly (tests/test_oracle_golden.py).
 * J in [2, 8]; SD_ERR_OVERFLOW if T*C(n-1,J) >= 2^63.
 * `ws`/`ws_bytes`: device scratch of at least sd_mbd_workspace_bytes(...).
 */
size_t sd_mbd_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int J, int algo);
int sd_mbd_counts(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn,
                  const int64_t *targets, int64_t m, int J, int algo,
                  int64_t *out, void *ws, size_t ws_bytes, void *stream);

/* Same totals for a CONTIGUOUS block of targets [target_begin, target_begin + m) -- the form the
 * target-sharded multi-GPU path uses (rank r owns one block of curves of the gathered set).  Lets the
 * chunked rank kernel search only the chunks that hold targets. */
int sd_mbd_counts_range(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn,
                        int64_t target_begin, int64_t m, int J, int algo,
                        int64_t *out, void *ws, size_t ws_bytes, void *stream);

/* The same totals as TWO-LIMB unsigned integers for problems whose totals do not fit int64 (sd_mbd_counts returns
 * SD_ERR_OVERFLOW there: J >= 4 at n = 10^5, or very long T): out[(q*(J-1) + (j-2))*2 + {0,1}] = (low, high) 64 bits
 * of sum_t contained_j.  Requires J * C(n-1, J) < 2^63 (one timepoint's count fits 64 bits); the timepoints are
 * processed in chunks whose totals fit int64 and added with carry.  Workspace: sd_mbd_wide_workspace_bytes. */
size_t sd_mbd_wide_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int J, int algo);
int sd_mbd_counts_wide(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn,
                       const int64_t *targets, int64_t m, int J, int algo,
                       uint64_t *out, void *ws, size_t ws_bytes, void *stream);

/* Band totals of m EXTERNAL curves Q (T x m, time-major dense) with respect to the n curves of X (time-major
 * dense, st = n, sn = 1): every curve of X is an "other".  This is what the reference's homogeneity
 * coefficients do |G| times with a temporary column (homogeneity.py:101-112,125-128: append g to F, call
 * FunctionalDepth(to_compute=[g]), drop g) -- here one launch for all of G.
 * out[q*(J-1)+(j-2)] = sum_t #{j-subsets of X's curves whose band contains Q[:,q] at t};
 * depth of g within F u {g} = sum_j out/T / C(n+1, j) on the host (_functional.py:229,253). */
int sd_mbd_external_counts(const double *X, int64_t T, int64_t n, const double *Q, int64_t m, int J,
                           int64_t *out, void *ws, size_t ws_bytes, void *stream);
/* Workspace for sd_mbd_external_counts.  With at least this much the call ranks the targets through a per-row bucket
 * structure (O(n + m) per timepoint, n <= 16384, J <= 3); with T*4 + 256 bytes it still works (pairwise, O(n m)). */
size_t sd_mbd_external_workspace_bytes(int64_t T, int64_t n, int64_t m, int J);

/* The same for the reference's default relax=False, J = 2: out[q] = number of pairs of X's curves whose band contains
 * Q[:,q] at EVERY timepoint (`c // T`, _containment.py:80); depth of g within F u {g} = out / C(n+1, 2).  One launch for
 * all of G (complement matching, see sd_bd_strict_counts). */
size_t sd_bd_strict_external_workspace_bytes(int64_t T, int64_t n, int64_t m);
int sd_bd_strict_external_counts(const double *X, int64_t T, int64_t n, const double *Q, int64_t m, int64_t *out, void *ws,
                                 size_t ws_bytes, void *stream);

/* Band totals of one target inside an explicit subset of the curves, for nb (subset, target) pairs in one launch:
 * the K-block sampled estimator (_samplefunctionaldepth, _functional.py:170-182) evaluates
 * _univariate_band_depth on n*K small blocks.  X time-major dense (st = n, sn = 1).
 * members: int32[nb*bs] column indices, -1 = padding; target: int32[nb], each a member of its block.
 * out[k*(J-1)+(j-2)] = sum_t #{j-subsets of the block's OTHER members whose band contains the target at t}.
 * Host: depth = sum_j out/T / C(block size, j). */
int sd_mbd_subset_counts(const double *X, int64_t T, int64_t n, const int32_t *members, int64_t nb, int bs,
                         const int32_t *target, int J, int64_t *out, void *stream);

/* The same estimator with the reference's default relax=False (`c // T`, _containment.py:80), J = 2: the number of pairs
 * of the block's OTHER members whose band contains the target at EVERY timepoint, for nb (subset, target) pairs in one
 * launch (a workgroup per pair, the block's masks in LDS).  Arguments as sd_mbd_subset_counts; out: int64[nb].
 * Host: depth = out / C(block size, 2).  Blocks whose masks do not fit the LDS (sd_bd_strict_subset_supported == 0:
 * bs * (2 * ceil(T/32) + 2) * 4 bytes > ~158 KB) keep them in the workspace instead
 * (sd_bd_strict_subset_workspace_bytes; 0 when the LDS suffices, ws may then be NULL). */
size_t sd_bd_strict_subset_workspace_bytes(int64_t T, int64_t nb, int bs);
int sd_bd_strict_subset_counts(const double *X, int64_t T, int64_t n, const int32_t *members, int64_t nb, int bs,
                               const int32_t *target, int64_t *out, void *ws, size_t ws_bytes, void *stream);
int sd_bd_strict_subset_supported(int64_t T, int bs);

/* Finest-granularity form of K1 (tests, diagnostics): AB[(q*T + t)*2 + {0,1}] =
 * (#curves strictly above, #strictly below) target q at t, as uint32. */
int sd_above_below(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn,
                   const int64_t *targets, int64_t m, uint32_t *AB,
                   void *ws, size_t ws_bytes, void *stream);

/* ---- K3: strict band depth (relax=False), J = 2 ------------------------------
 * Replaces: the same loop (_functional.py:246-251) with `containment // len(curve)`
 * (_containment.py:80): a pair counts only if its band contains the target at
 * EVERY timepoint.  out[q] = number of such unordered pairs of other curves.
 * depth = out / C(n,2) on the host.
 * How the pairs are counted (always the same integers):
 *   T <= 5 (point clouds as `FunctionalDepth([points.T])`: the L-infinity / box depth), any n: per target one pass over
 *     the curves into 3^T / 4^T state classes and a class transform -- O(n) per target;
 *   T = 6 ... 8 without NaN anywhere, any n: the same (3^T classes; "NaN anywhere" is a flag the call reads back from the
 *     device: for these T the call waits on `stream` once before it launches the counting;
 *     sd_bd_strict_nanfree_workspace_bytes is the workspace such data needs).  With NaN: as below;
 *   n <= 131 071: curves that are strictly above or below the target at every timepoint ("clean") pair up exactly when
 *     their above-masks are complements, so those pairs are counted by grouping masks; pairs with a curve that ties
 *     with the target or holds NaN are tested one by one (only the targets that have such curves);
 *   beyond: every pair is tested; calls that would need more than 2e14 pair tests are refused (SD_ERR_UNSUPPORTED).
 * NaN in the target: out[q] = 0; NaN in another curve: it joins both masks (pandas' skipna min / max).
 * The workspace holds up to 16 GiB of masks for a batch of targets when n is large (sd_bd_strict_workspace_bytes: the
 * RECOMMENDED size).  A caller short of memory may pass less, down to sd_bd_strict_min_workspace_bytes (one target per
 * batch): the launcher sizes its batches to what it is given -- same integers, more launches.
 */
size_t sd_bd_strict_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m);
size_t sd_bd_strict_min_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int J);
/* The size for a caller who knows that X holds no NaN (J = 2): a few KB for 6 ... 8 timepoints (the state classes need a flag,
 * none of the mask pipeline's buffers), sd_bd_strict_workspace_bytes otherwise.  Passing it for data WITH NaN is safe: the
 * call returns SD_ERR_WORKSPACE. */
size_t sd_bd_strict_nanfree_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m);
int sd_bd_strict_counts(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn,
                        const int64_t *targets, int64_t m,
                        int64_t *out, void *ws, size_t ws_bytes, void *stream);

/* ---- K3b: strict band depth, general J (subset enumeration over bit masks) ----
 * out[q*(J-1)+(j-2)] = #{j-subsets of others containing target q at every t}.
 * J in [2, 4]; work grows as C(n-1,J) per target.
 */
size_t sd_bd_strict_j_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int J);
int sd_bd_strict_j_counts(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn,
                          const int64_t *targets, int64_t m, int J,
                          int64_t *out, void *ws, size_t ws_bytes, void *stream);

/* ---- K5: L1 (spatial) depth of a point cloud ----------------------------------
 * Replaces: _L1_depth (_pointcloud.py:125-150).  P is n x d row-major (rows =
 * points).  out[q] = 1 - || sum_{y != x} (y-x)/||x-y|| || / n  (fp64; coincident
 * points give NaN like the reference's 0/0).
 */
int sd_l1_depth(const double *P, int64_t n, int d, const int64_t *targets, int64_t m,
                double *out, void *stream);

/* The same depth for m EXTERNAL points Q (m x d): every row of P is an "other" and the sample counts n + 1 points --
 * what the reference's point-cloud homogeneity does once per point of G with a temporary row
 * (homogeneity.py:172-175,183-186: append g to F, PointcloudDepth(to_compute=[g]), drop g); here one launch for all. */
int sd_l1_external_depth(const double *P, int64_t n, int d, const double *Q, int64_t m, double *out, void *stream);
/* ... and inside explicit BLOCKS of rows, nb (block, target) pairs in one launch: the K-block sampled estimator
 * (_samplepointwisedepth, _pointcloud.py:107-121) calls _pointwisedepth on len(to_compute) * (n // K) samples.
 * members: int32[nb*bs] row indices, -1 = padding AT THE END of a block; in every block the OTHER rows first and the
 * target LAST.  A block's members are the entries before its first -1 (so for every block form of a point cloud below:
 * simplex, Oja, halfspace, exact halfspace); a block without members gives NaN.
 * out[k] = 1 - ||sum over the block's others|| / (block size). */
int sd_l1_subset_depth(const double *P, int64_t n, int d, const int32_t *members, int64_t nb, int bs, double *out,
                       void *stream);

/* ---- K4: simplex containment counts ---------------------------------------------
 * Replaces: _is_in_simplex (_containment.py:138-176, an LP feasibility test
 * through scipy.optimize.linprog) inside
 *   - _pointwisedepth's subset loop (_pointcloud.py:50-54): sd_pointcloud_simplex_counts,
 *     P n x d row-major, out[q] = #{(d+1)-subsets of the other n-1 points whose
 *     simplex contains point q}; depth = out / C(n,d+1) on the host;
 *   - _simplex_depth / _simplex_containment (_functional.py:281-285,
 *     _containment.py:130-136): sd_multi_simplex_counts, P n x T x d row-major
 *     (curve, timepoint, feature); per target and (d+1)-subset of the other
 *     curves c = #{t: x_q(t) in simplex}; out[q] = sum c (relax != 0) or
 *     sum [c == T] (relax == 0); depth = out / (T or 1) / C(n-1,d+1) on the host.
 * Containment = the closed simplex (degenerate point sets allowed) with
 * feasibility tolerance `tol` on the barycentric coordinates (1e-7 mirrors the
 * LP solver's default).  d in [1, 8].
 * subset enumeration is exhaustive: C(n-1,d+1) per target must be < 2^62.
 */
int sd_pointcloud_simplex_counts(const double *P, int64_t n, int d,
                                 const int64_t *targets, int64_t m, double tol,
                                 int64_t *out, void *stream);
int sd_multi_simplex_counts(const double *P, int64_t n, int64_t T, int d,
                            const int64_t *targets, int64_t m, int relax, double tol,
                            int64_t *out, void *stream);

/* External targets / explicit blocks, as for sd_l1_external_depth / sd_l1_subset_depth above:
 *   out[q] = #{(d+1)-subsets of ALL n rows of P whose simplex contains Q[q]}; depth = out / C(n+1, d+1) on the host
 *   (_pointcloud.py:38,56 with the temporary row counted: homogeneity.py:172-175,183-186);
 *   out[k] = #{(d+1)-subsets of block k's other rows whose simplex contains the block's target (its last row)};
 *   depth = out / C(block size, d+1) (_pointcloud.py:107-121 -> :50-56 on the sample). */
int sd_pointcloud_simplex_external_counts(const double *P, int64_t n, int d, const double *Q, int64_t m, double tol,
                                          int64_t *out, void *stream);
int sd_pointcloud_simplex_subset_counts(const double *P, int64_t n, int d, const int32_t *members, int64_t nb, int bs,
                                        double tol, int64_t *out, void *stream);

/* Seeded uniform subset-sampling estimators for sizes where exhaustive
 * enumeration is impossible (BASELINE.json configs 4 and 5; not in the
 * reference).  For each target, `samples` (d+1)-subsets of the
 * other items are drawn with a counter-based generator (keys below); out[q] = number of
 * containing simplices (pointcloud) or sum over samples of c / [c == T] (multi).
 */
/* Round 4: sample s is ONE (d+1)-subset of all n items for every target (generator keyed by (seed, s)); a target that is
 * itself a member gets that member replaced by an item drawn with the generator keyed by (seed, target, s) -- every target
 * sees `samples` uniform subsets of the other items, and the subset's elimination is shared by all targets (each target only
 * carries its right-hand side through the recorded row operations: the same barycentric coordinates bit for bit).
 * ws / ws_bytes: optional (NULL / 0 allowed) records of a batch of (timepoint, sample) pairs, sd_simplex_sampled_workspace_bytes;
 * with it the factorisation and the replay are two kernels (d >= 4: several times faster), without it one. */
size_t sd_simplex_sampled_workspace_bytes(int64_t n, int64_t T, int d, int64_t samples);
int sd_pointcloud_simplex_sampled(const double *P, int64_t n, int d,
                                  const int64_t *targets, int64_t m, double tol,
                                  int64_t samples, uint64_t seed, int64_t *out,
                                  void *ws, size_t ws_bytes, void *stream);
int sd_multi_simplex_sampled(const double *P, int64_t n, int64_t T, int d,
                             const int64_t *targets, int64_t m, int relax, double tol,
                             int64_t samples, uint64_t seed, int64_t *out,
                             void *ws, size_t ws_bytes, void *stream);

/* ---- K6: componentwise band containment of multivariate curves ('r2_enum') --------
 * Fills: _r2_enum_containment (_containment.py:83-103), which the reference declares -- "treat each component in the
 * vector valued function as a real valued function ... if all the components are contained ... the function is
 * contained" -- and leaves as `raise NotImplementedError`; built as the predicate of _univariate_band_depth's pair
 * loop (_functional.py:238-253), relax=True; J = 2 here, J <= 4 below.  P is n x T x d row-major (curve, timepoint,
 * feature), NaN-free.
 *   out[q] = sum_t #{pairs {a,b} of the other curves: for every feature f,
 *                    min(a_f(t), b_f(t)) <= x_q,f(t) <= max(a_f(t), b_f(t))};   depth = out / T / C(n,2) on the host
 * (d = 1 gives sd_mbd_counts' totals).  The strict form (contained at every t) is sd_bd_strict_j_counts over the
 * T*d component series of each curve (st = 1, sn = T*d) and needs no entry point of its own.
 * n <= 65535 and n*d*2 + 8*3^d bytes of LDS (config 4: 5000 curves, d = 8: 132 KB). */
size_t sd_multi_band_workspace_bytes(int64_t n, int64_t T, int d);
int sd_multi_band_counts(const double *P, int64_t n, int64_t T, int d, const int64_t *targets, int64_t m,
                         int64_t *out, void *ws, size_t ws_bytes, void *stream);
/* The same predicate for the j-subsets of the other curves, every j = 2 .. J in one pass (J in [2, 4]): the lines
 * _containment.py:83-103 would fill inside _univariate_band_depth's loop over j (_functional.py:238-253), relax=True.
 *   out[q*(J-1) + j-2] = sum_t #{j-subsets S of the other curves: for every feature f,
 *                               min_{a in S} a_f(t) <= x_q,f(t) <= max_{a in S} a_f(t)};
 *   depth = sum_j out[q][j-2] / T / C(n,j) on the host, n counting the target (d = 1 gives sd_mbd_counts' totals).
 * Counted without enumerating subsets: S fails at (t, f) iff all its members are strictly above x_f(t) or all strictly
 * below, so with p in {don't care, all above, all below}^d and N_p = number of other curves matching p,
 *   containing j-subsets at t = sum_p (-1)^(constrained features of p) C(N_p, j).
 * Input limits and workspace (sd_multi_band_workspace_bytes) are those of sd_multi_band_counts.  SD_ERR_UNSUPPORTED for
 * J outside [2, 4]; SD_ERR_OVERFLOW, before any launch, if T*C(n-1,J) >= 2^63 (as sd_mbd_counts). */
int sd_multi_band_j_counts(const double *P, int64_t n, int64_t T, int d, const int64_t *targets, int64_t m, int J,
                           int64_t *out /* m*(J-1) */, void *ws, size_t ws_bytes, void *stream);

/* ---- K7: Oja volume sums of a point cloud ------------------------------------------------
 * Replaces: the subset loop of _oja_depth (_pointcloud.py:175-205, one scipy ConvexHull per simplex).  P is n x d
 * row-major.  out[q] = sum over d-subsets S of the target's others of vol(conv(S u {x})) = |det[x_s - x]| / d!
 * (fp64, raw sums); depth = out / ConvexHull(sample).volume on the host.  Degenerate simplices add their volume (~0).
 *   sd_oja_volume_sums:          others = the n - 1 rows other than targets[q] (NULL = all, m == n);
 *   sd_oja_external_volume_sums: d-subsets of ALL n rows of P against the external point Q[q] (m x d);
 *   sd_oja_subset_volume_sums:   blocks of rows, members int32[nb*bs], -1 padded at the end, the block's others
 *                                first and its target LAST (the K-block sampled estimator).
 * A target's result is bitwise independent of m, of the other targets and of the run.  d in [1, 8];
 * SD_ERR_OVERFLOW if C(others, d) >= 2^62; SD_ERR_UNSUPPORTED for 2^31 or more others or if m * C(others, d) > 1e14
 * (hours of work).  Every launch is bounded (at most 2^32 >> max(0, d - 5) subset volumes). */
int sd_oja_volume_sums(const double *P, int64_t n, int d, const int64_t *targets, int64_t m,
                       double *out, void *stream);
int sd_oja_external_volume_sums(const double *P, int64_t n, int d, const double *Q, int64_t m,
                                double *out, void *stream);
int sd_oja_subset_volume_sums(const double *P, int64_t n, int d, const int32_t *members, int64_t nb, int bs,
                              double *out, void *stream);

/* ---- K8: probabilistic depths (normal distributions, Poisson curves) ---------------------------
 * Replaces: the two exported functions of _uncertainty.py.  Both return UNNORMALISED fp64 sums; the host divides.
 *   sd_prob_normal_sums:  the (target, pair) quad loop of _normal_depth (:101-121).  mu, sigma: n doubles (device).
 *       out[q] = sum over pairs i < j of the others of k = targets[q] of int (Phi_i - Phi_k Phi_j) phi_k
 *              = sum_{m != k} Phi(h) ((n - 1 - m) - [k > m]) - sum_{m != k} Phi2(0, h; rho) (m - [k < m]),
 *       h = (mu_k - mu_m) / sqrt(sigma_m^2 + sigma_k^2), rho = sigma_k / sqrt(2 (sigma_m^2 + sigma_k^2));
 *       depth = out / C(n, 2).  Needs finite mu and finite sigma > 0 (the host checks the values).
 *   sd_prob_poisson_sums: the (target, pair, row) loop of _poisson_depth (:47-61) over
 *       _poisson_containment_simplified (:34-45).  lam: T x n row-major rates (device), row t = timepoint, column = curve.
 *       out[q] = sum_t sum_{z=1}^{lim-1} sum over column pairs i < j, both != f = targets[q], of
 *                P(X_f = z) P(X_i <= z) P(X_j >= z),  X_c ~ Poisson(lam[t][c]);
 *       depth = out / C(T, 2).  Needs finite lam >= 0 (the host checks the values).  lim <= 1: zeros.
 * targets: m int64 indices (device; the engine checks their range on the host), NULL = all (m == n).  A target's
 * result is bitwise independent of m, of the other targets and of how the call is cut into launches (no atomics).
 * SD_ERR_INVALID for NULL pointers or negative sizes; SD_ERR_OVERFLOW if n * m (normal) or T * n * lim (Poisson)
 * overflows int64; SD_ERR_UNSUPPORTED beyond 10^14 of them (hours of work).  Every launch is bounded in work. */
int sd_prob_normal_sums(const double *mu, const double *sigma, int64_t n, const int64_t *targets, int64_t m,
                        double *out, void *stream);
int sd_prob_poisson_sums(const double *lam, int64_t T, int64_t n, int64_t lim, const int64_t *targets, int64_t m,
                         double *out, void *stream);

/* ---- K9: band depth of curves under Gaussian noise (ProbabilisticDepth) -----------------------
 * No reference code (its prob_depth.py is empty); the quantity is the expected J = 2 band depth of random curves.
 * mu, var: T x n row-major (device), row t = timepoint, column = curve; X_c(t) ~ N(mu[t][c], var[t][c]), independent,
 * var = 0 a point mass.  For target i = targets[q] and a pair {j, k} of its others,
 *     p_ijk(t) = P(min(X_j, X_k) <= X_i <= max(X_j, X_k))
 *              = Phi(h_j) + Phi(h_k) - 2 Phi2(h_j, h_k; rho),  h_c = (mu_i - mu_c) / s_c, s_c = sqrt(var_i + var_c),
 *                rho = var_i / (s_j s_k)  (Phi2 by Genz's BVND, evaluated as the two orthants where D_j, D_k differ in sign)
 *     out[q] = sum_{j<k} sum_t p_ijk(t)   (relax != 0)      out[q] = sum_{j<k} prod_t p_ijk(t)   (relax == 0)
 * depth = out / T / C(n', 2) (relax) or out / C(n', 2), n' counting the target.  Degenerate cases are exact:
 * var_i = 0 gives p = 1 - a_j a_k - b_j b_k (a_c = P(X_c > mu_i), b_c = P(X_c < mu_i)); var_j = var_k = 0 < var_i gives
 * Phi(hmax) - Phi(hmin); with every variance zero p is 0 or 1 and out equals the integer band counts of
 * sd_mbd_counts / sd_bd_strict_counts.
 * members: NULL = every other column; otherwise m x bs int32 (device) padded with -1, row q = the block of target q
 * (the target is skipped where listed).  targets: m int64 (device; the engine checks ranges on the host), NULL = all.
 * A target's result is bitwise independent of m, of the other targets and of how the call is cut into launches.
 * SD_ERR_INVALID for NULL pointers or negative sizes; SD_ERR_OVERFLOW if m * C(positions, 2) * T overflows int64;
 * SD_ERR_UNSUPPORTED beyond 10^14 pair evaluations.  Both before any device work.  Every launch is bounded in work. */
int sd_prob_band_sums(const double *mu, const double *var, int64_t T, int64_t n, const int64_t *targets, int64_t m,
                      const int32_t *members, int bs, int relax, double *out, void *stream);

/* ---- K10: halfspace (Tukey) depth of a point cloud over a fixed direction set ----------------
 * No reference code (the reference has no halfspace depth).  P is n x d row-major, U is k x d row-major (both device).
 *   z_r(x)   = ((x_0 u_r0 + x_1 u_r1) + x_2 u_r2) + ...   features in increasing order, every product and every sum
 *              rounded separately to fp64 (no FMA): a numpy loop over the features gives the same bits;
 *   ge_r(q)  = #{i : z_r(p_i) >= z_r(q)},  le_r(q) = #{i : z_r(p_i) <= z_r(q)}   (q itself and every tie counted);
 *   out[q]   = min over r of min(ge_r(q), le_r(q))   (one direction serves u and -u);   depth = out / n on the host.
 * This is the directional (random Tukey) depth: an upper bound of the exact halfspace depth for d >= 2, exact for
 * d = 1 with the direction (1.0).  Projections must not be NaN (finite data and directions: the host checks).
 *   sd_halfspace_counts:          the sample is P, targets: m int64 row indices (device), NULL = all (m == n).  Every
 *       row is ranked in every direction whatever m is: projection (a kc x n fp64 matrix per chunk of kc directions),
 *       sort with index payload (tiles of 2048 in LDS, then merge passes), ranks from the sorted rows, running minimum --
 *       O(k n (d + log n)), no all-pairs pass.  kc follows from ws_bytes; sd_halfspace_workspace_bytes recommends a size,
 *       sd_halfspace_min_workspace_bytes is the floor (one direction per chunk: about 28 n bytes), SD_ERR_WORKSPACE
 *       below it.  The counts do not depend on the workspace size (integer minima).
 *   sd_halfspace_pairwise_counts: the same counts by the pairwise kernel, O(m n k d) (cross-checks, timing).
 *   sd_halfspace_external_counts: m external points Q (m x d, device) against P; the sample of Q[q] is P u {Q[q]}: the
 *       counts are over n + 1 points (Q[q] counts itself once), depth = out / (n + 1).  Pairwise kernel.
 *   sd_halfspace_subset_counts:   blocks of rows, members int32[nb*bs], -1 padded at the end, the block's target LAST;
 *       the block (target included) is the sample: depth = out / block size.  An empty block gives 0.  Pairwise kernel.
 * SD_ERR_INVALID for NULL pointers or n, d, k < 1; SD_ERR_UNSUPPORTED for d > 8, 2^31 or more points, or more than
 * 10^14 projections and comparisons (k n (d + log2 n), resp. m n k d).  All before any device work.  Every launch is
 * bounded in work. */
size_t sd_halfspace_workspace_bytes(int64_t n, int d, int64_t k);
size_t sd_halfspace_min_workspace_bytes(int64_t n, int d, int64_t k);
int sd_halfspace_counts(const double *P, int64_t n, int d, const double *U, int64_t k, const int64_t *targets, int64_t m,
                        int64_t *out, void *ws, size_t ws_bytes, void *stream);
int sd_halfspace_pairwise_counts(const double *P, int64_t n, int d, const double *U, int64_t k, const int64_t *targets,
                                 int64_t m, int64_t *out, void *stream);
int sd_halfspace_external_counts(const double *P, int64_t n, int d, const double *U, int64_t k, const double *Q, int64_t m,
                                 int64_t *out, void *stream);
int sd_halfspace_subset_counts(const double *P, int64_t n, int d, const double *U, int64_t k, const int32_t *members,
                               int64_t nb, int bs, int64_t *out, void *stream);

/* ---- K11: exact halfspace (Tukey) depth of a point cloud in the plane ------------------------
 * No reference code.  P is n x 2 row-major fp64 (device).  For a target q and every sample point p_i:
 *   v_i   = (fl(p_i0 - q0), fl(p_i1 - q1))   one rounded fp64 subtraction per component;
 *   c0    = #{i : v_i = (0, 0)}   (q itself when it is a row of the sample; an external q adds one);
 *   cross(a, b) = a0 b1 - a1 b0,  dot(a, b) = a0 b0 + a1 b1,  of which only the EXACT signs are used;
 *   for every nonzero v_j, over the nonzero v_k:
 *     L_j = #{cross(v_j, v_k) > 0}              R_j = #{cross(v_j, v_k) < 0}
 *     S_j = #{cross = 0 and dot > 0} (j itself)  O_j = #{cross = 0 and dot < 0}
 *   out[q] = c0 + min over j of min(L_j + O_j, R_j + S_j, L_j + S_j, R_j + O_j);   out[q] = c0 when no v is nonzero.
 * The four candidates are the open sides of the line through q along v_j turned a hair to either side; the count of a
 * closed halfplane is upper semicontinuous in its direction, so the minimum over all closed halfplanes through q is
 * reached at such lines: out / n is the halfspace depth of q in the sample, not a bound of it.
 * Predicate: sign(a b - c d) from p1 = fl(a b), p2 = fl(c d): where p1 != p2 the sign of p1 - p2 (rounding is monotone),
 * otherwise, while |p1| >= 2^-900, the sign of e1 - e2 with the exact rounding errors e = fma(a, b, -p) (fp64 numbers
 * there), and below that -- zero and underflowing products included, where the fma would lose the errors -- the signs of
 * the products, their exponent sums and the same comparison on the frexp mantissas.  Exact for every finite input whose
 * products do not overflow: the data must be finite with |coordinate| <= 2^500 (the host layer raises otherwise); there
 * is NO lower limit on the coordinate differences, subnormal ones included.  The sign of the rounded cross product is
 * not a substitute (it is wrong for nearly collinear triples).
 * algo: 0 = auto, 1 = sweep, 2 = pairwise; the same integers from both.
 *   sweep     one workgroup per target: the nonzero v in LDS (16 bytes each), each read through its image in the
 *             half-plane y > 0 or (y = 0, x > 0) (exact negation, the flip recomputed from v), sorted by angle with the
 *             predicate as comparator; cuts where neighbours have cross != 0 and after the last element; for a cut after
 *             position s, A = #{i <= s unflipped} + #{i > s flipped}, B likewise with the flags exchanged;
 *             out = c0 + min over cuts of min(A, B).  Capacity tiers of 64 / 512 / 2048 / 8192 sample points
 *             (64 / 256 / 512 / 1024 threads); samples of at most 8192 points.  O(n log^2 n) per target.
 *   pairwise  the definition as it stands, O(n^2) predicate pairs per target: any n below 2^31.
 *   auto      the sweep up to 8192 sample points, the pairwise kernel above.
 *   sd_halfspace2_counts:          the sample is P; targets: m int64 row indices (device), NULL = all (m == n).
 *   sd_halfspace2_external_counts: m external points Q (m x 2, device); the sample of Q[q] is P u {Q[q]}, n + 1 points,
 *       Q[q] adds one to c0; depth = out / (n + 1).
 *   sd_halfspace2_subset_counts:   blocks of rows, members int32[nb*bs], -1 padded at the end, the block's target LAST;
 *       the block (target included) is the sample: depth = out / block size.  An empty block gives 0.
 * SD_ERR_INVALID for NULL pointers, n < 1, bs < 1 or an unknown algo; SD_ERR_UNSUPPORTED for 2^31 or more points, for
 * algo = 1 on a sample (n, resp. bs) above 8192 points, or beyond 10^14 predicate evaluations on the route that would run
 * (pairwise: m n^2; sweep: m (C / 2) log2 C (log2 C + 1) / 2 at capacity tier C).  All before any device work.  Every
 * launch is bounded in work. */
int sd_halfspace2_counts(const double *P, int64_t n, const int64_t *targets, int64_t m, int algo, int64_t *out,
                         void *stream);
int sd_halfspace2_external_counts(const double *P, int64_t n, const double *Q, int64_t m, int algo, int64_t *out,
                                  void *stream);
int sd_halfspace2_subset_counts(const double *P, int64_t n, const int32_t *members, int64_t nb, int bs, int algo,
                                int64_t *out, void *stream);

/* ---- K12: projection depth (Stahel-Donoho outlyingness) of a point cloud over a fixed direction set ----
 * No reference code.  P is n x d row-major, U is k x d row-major (both device), d <= 8.  For a sample S of N points:
 *   z_r(x)    = K10's projection, the same bits (features in increasing order, products and sums rounded separately);
 *   median(v) = s[(N-1)/2] for N odd, (s[N/2-1] + s[N/2]) * 0.5 for N even (s = v sorted; the sum rounded, then the
 *               product rounded);
 *   med_r     = median(z_r(S));  mad_r = median(|z_r(p_i) - med_r|) (one rounded subtraction, the sign cleared; no
 *               1.4826 factor);
 *   o_r(q)    = |z_r(q) - med_r| / mad_r, one correctly rounded division; a numerator of 0 gives 0 whatever mad_r is, a
 *               numerator above 0 with mad_r = 0 gives +inf;
 *   out[q]    = max over r of o_r(q);   depth = 1 / (1 + out) on the host.
 * Every step is one correctly rounded fp64 operation or an order statistic: a numpy restatement gives the same bits.
 * The data and the directions must be finite with magnitudes of at most 2^500 (the host checks), so nothing overflows
 * on the way to the division and no NaN arises.
 *   sd_projection_outlyingness:          S = P, targets: m int64 row indices (device), NULL = all (m == n).  Per chunk
 *       of kc directions: K10's projection and sort, med and MAD by O(log n) selection from the sorted rows, then one
 *       evaluation per (target, direction).  kc follows from ws_bytes; sd_projection_workspace_bytes recommends a size,
 *       sd_projection_min_workspace_bytes is the floor (one direction per chunk: about 24 n bytes), SD_ERR_WORKSPACE
 *       below it.  The result does not depend on the workspace size (the maximum is exact).
 *   sd_projection_external_outlyingness: m external points Q (m x d, device); S = P u {Q[q]}, N = n + 1: every external
 *       point has a median and a MAD of its own, selected from P's sorted rows with Q[q]'s projection inserted.
 *   sd_projection_subset_outlyingness:   blocks of rows, members int32[nb*bs], -1 padded at the end, the block's target
 *       LAST; S = the block's members.  bs <= 2048 (a block is sorted in LDS).  An empty block gives 0.
 * SD_ERR_INVALID for NULL pointers or n, d, k, bs < 1; SD_ERR_UNSUPPORTED for d > 8, bs > 2048, 2^31 or more points, or
 * more than 10^14 projections and comparisons.  All before any device work.  Every launch is bounded in work. */
size_t sd_projection_workspace_bytes(int64_t n, int d, int64_t k);
size_t sd_projection_min_workspace_bytes(int64_t n, int d, int64_t k);
int sd_projection_outlyingness(const double *P, int64_t n, int d, const double *U, int64_t k, const int64_t *targets,
                               int64_t m, double *out, void *ws, size_t ws_bytes, void *stream);
int sd_projection_external_outlyingness(const double *P, int64_t n, int d, const double *U, int64_t k, const double *Q,
                                        int64_t m, double *out, void *ws, size_t ws_bytes, void *stream);
int sd_projection_subset_outlyingness(const double *P, int64_t n, int d, const double *U, int64_t k, const int32_t *members,
                                      int64_t nb, int bs, double *out, void *stream);

/* ---- K13: exact simplicial depth of a point cloud in the plane (angular sweep) ---------------
 * The reference's point-cloud simplex depth (_pointcloud.py:14-66) for d = 2, decided with exact signs instead of K4's
 * tolerance.  P is n x 2 row-major fp64 (device).  For a target x, over its OTHERS p_i (the sample without the target's
 * own row: all n rows for an external point, a block's members before the last for a block), m of them:
 *   v_i   = (fl(p_i0 - x0), fl(p_i1 - x1))   one rounded fp64 subtraction per component, as in K11;
 *           others with v_i = (0, 0) are duplicates of x: every triple that holds one of them contains x;
 *   cross(a, b) = a0 b1 - a1 b0,  dot(a, b) = a0 b0 + a1 b1,  of which only the EXACT signs are used (K11's predicate);
 *   for every nonzero v_j, counting over the nonzero v_k:
 *     e_j = #{k : cross(v_j, v_k) > 0} + #{k later than j in sample order : cross(v_j, v_k) = 0 and dot(v_j, v_k) > 0};
 *   out[x] = C(m, 3) - sum over j of C(e_j, 2).
 * out[x] is the number of triples of others whose closed convex hull (a segment or a point for a degenerate triple)
 * contains x.  A triple misses x exactly when its three vectors are nonzero and fit in an open half-plane; the sum counts
 * such triples once each, at their clockwise-most member, members of one direction ordered by position in the sample.  The
 * sum does not depend on that tie order: over a direction class of size s with common L = #{cross > 0} it is
 * sum_{r < s} C(L + r, 2), so the sweep may order a class as it likes.
 * depth = out / C(N, 3) on the host, N the sample size INCLUDING the point (K4's normalisers): n for a row target, n + 1
 * for an external point, the block size for a block.
 * Predicate domain as K11: finite data with |coordinate| <= 2^500 (the host layer raises otherwise); no lower limit on
 * the coordinate differences.
 * algo: 0 = auto, 1 = sweep, 2 = pairwise; the same integers from both.
 *   sweep     one workgroup per target: K11's compaction, sort and flag prefix over the nonzero vectors of the others;
 *             groups are runs of sorted neighbours with cross = 0; the element at position i of group [g0, g1] with flip
 *             flag f has L = #{positions > g1 with flag f} + #{positions < g0 with flag != f} and rank r among the
 *             same-flag elements of its group; sum of C(L + r, 2) in 64 bits.  Capacity tiers of 64 / 512 / 2048 / 8192
 *             others (64 / 256 / 512 / 1024 threads); at most 8192 others.  O(m log^2 m) per target, whatever the ties.
 *   pairwise  the definition as it stands, O(m^2) predicate pairs per target.
 *   auto      the sweep up to 8192 others, the pairwise kernel above.
 *   sd_simplicial2_counts:          targets: m int64 row indices (device), NULL = all (m == n); n - 1 others each.
 *   sd_simplicial2_external_counts: m external points Q (m x 2, device); n others each.
 *   sd_simplicial2_subset_counts:   blocks of rows, members int32[nb*bs], -1 padded at the end, the block's target LAST;
 *       at most bs - 1 others.  An empty block, and any target with fewer than 3 others, gives 0.
 * SD_ERR_INVALID for NULL pointers, n < 1, bs < 1 or an unknown algo; SD_ERR_UNSUPPORTED for 2^31 or more points, for
 * algo = 1 with more than 8192 others, where C(others, 3) does not fit int64 (more than 3 810 779 others), or beyond 10^14
 * predicate evaluations on the route that would run (K11's formulas over the others).  All before any device work.
 * Every launch is bounded in work. */
int sd_simplicial2_counts(const double *P, int64_t n, const int64_t *targets, int64_t m, int algo, int64_t *out,
                          void *stream);
int sd_simplicial2_external_counts(const double *P, int64_t n, const double *Q, int64_t m, int algo, int64_t *out,
                                   void *stream);
int sd_simplicial2_subset_counts(const double *P, int64_t n, const int32_t *members, int64_t nb, int bs, int algo,
                                 int64_t *out, void *stream);

/* ---- K14: integrated rank depths of curves (Fraiman-Muniz, MEI / MHI, half-region, univariate halfspace) ----
 * No reference code (the reference has only band depths for curves).  X is T x n fp64 in either layout, finite or
 * +-inf.  NaN is NOT supported: the counts of a row that holds one are unspecified (the host layer refuses NaN).
 * For a target q at timepoint t, over the other n - 1 curves:
 *   A = #{y : y(t) > x_q(t)},  B = #{y : y(t) < x_q(t)}   (ties in neither; so #{y <= x} = n - A and #{y >= x} = n - B
 *   with the target counting itself in both);
 * out[q] is the record of five non-negative int64
 *   SA = sum_t A,   SB = sum_t B,   SF = sum_t |2 A - n|,   SM = sum_t max(A, B),   MM = max_t max(A, B),
 * and the depths are formed on the host in fp64, one expression each, the division last:
 *   Fraiman-Muniz         1 - SF / (2 n T)       mean over t of 1 - |1/2 - F_t(x(t))|, F_t the empirical CDF with "<=":
 *                                                F = (n - A) / n.  Not symmetric under x -> -x: the published definition;
 *   modified epigraph     (n T - SB) / (n T)     mean proportion of curves at or above x;
 *   modified hypograph    (n T - SA) / (n T)     mean proportion of curves at or below x;
 *   modified half-region  min of the two         (Lopez-Pintado & Romo 2011);
 *   integrated halfspace  (n T - SM) / (n T)     mean over t of the univariate Tukey depth min(#<=, #>=) / n;
 *   infimal halfspace     (n - MM) / n           its infimum over t.
 * Both routes form the same pairs (A, B) of every (row, curve) and one kernel folds them into the records:
 *   image (algo 1)  n <= 16 384: the rank kernel of K1+K2 in its pair-image mode, a batch of rows at a time (at most
 *                   2^16 rows and 1 GiB), u32 words B | A << 16, one streaming pass over 4 bytes per (row, curve);
 *   sort  (algo 2)  any n < 2^31: K10's sort with the curve's index as payload, a chunk of rows at a time; the rank of
 *                   every sorted position (runs of ties by binary search) stored as u64 B | A << 32 at the curve's
 *                   place, then the same fold.  O(T n log n).
 *   auto  (algo 0)  the image route up to 16 384 curves, the sort route above.
 * The batch and the chunk follow from ws_bytes: sd_rank_depth_workspace_bytes recommends a size,
 * sd_rank_depth_min_workspace_bytes is the floor (one row per batch: about 4 n bytes on the image route, 24 n on the
 * sort route, plus 8 T n for the time-major copy of a curve-major X).  sd_rank_depth_rows_per_batch says how many rows a
 * batch (a chunk) of a call with ws_bytes takes, 0 below the floor or for a shape or algo the call refuses: at the
 * recommended size all T rows in one batch whenever T is within the route's caps (image: 2^16 rows and a 1 GiB image;
 * sort: 2^23 values).  The integers do not depend on the workspace size.
 * targets: m int64 curve indices (device), NULL = all (m == n).  out: m x 5 int64 (device).
 * SD_ERR_INVALID for NULL X or out, T < 1, n < 2 or an unknown algo; SD_ERR_UNSUPPORTED for algo = 1 with n > 16 384 or
 * for 2^31 or more curves or timepoints; SD_ERR_WORKSPACE below the floor.  All before any device work. */
size_t sd_rank_depth_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int algo);
size_t sd_rank_depth_min_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int algo);
int64_t sd_rank_depth_rows_per_batch(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int algo, size_t ws_bytes);
int sd_rank_depth_sums(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const int64_t *targets, int64_t m,
                       int algo, int64_t *out, void *ws, size_t ws_bytes, void *stream);

/* ---- K15: extremal depth of curves (Narisetty & Nair, JASA 2016) ----
 * No reference code.  X is T x n fp64 in either layout, finite or +-inf; NaN is NOT supported (the host layer refuses
 * it).  For curve q at timepoint t, with K14's A and B over the other n - 1 curves (ties in neither):
 *   pointwise extremity  e_q(t) = |A - B|  in [0, n - 1]      (the paper's pointwise depth is 1 - e / n);
 *   v_q = the T values e_q(.) sorted in descending order;
 *   curve f is more extreme than or equal to g  iff  v_f >= v_g lexicographically.
 * This is the paper's ordering of the depth CDFs: compare Phi from the lowest depth level upward, and at the first
 * difference the larger Phi belongs to the more extreme curve.  The device returns one int64 per target,
 *   G_q = #{ i in the sample : v_i >=lex v_q }   (q itself and every curve with an identical vector are counted),
 * and the host forms ED = G / n in fp64 with one division: 1 for the deepest curve, equal depths for equal vectors.
 * Example: rows [1,2,3,4], [2,1,3,3], [1,3,2,4] (T = 3, n = 4) have e = (3,1,1,3), (1,3,2,2), (3,1,1,3), so
 * v = (3,3,1), (3,1,1), (2,1,1), (3,3,2), G = [2, 3, 4, 1], ED = [0.5, 0.75, 1, 0.25].
 * Stages: (1) the pair image of a batch of rows by K14's two routes -- algo 0 auto, 1 image (n <= 16 384), 2 sort, the
 * same boundary; (2) a transposing transform writes |A - B| of all n curves into the u32 matrix E, curve-major;
 * (3) every curve's row of E is sorted descending in LDS (padded with 0 to a power of two; at most 16 384 timepoints =
 * 64 KiB of keys) and its head packed into one u64: the first P = min(T, 64 / b) entries in fields of b bits, most
 * significant first, missing fields 0, b = max(16, bit width of n - 1), so P = 4 up to 65 536 curves, 3 up to 2^21,
 * 2 beyond; (4) each target counts the curves with a larger head and, where the heads are equal, compares the entries
 * P .. T - 1 to the first difference (equal to the end counts).
 * Workspace, in this order: the time-major copy of a curve-major X (8 T n bytes), E (4 T n), the heads (8 n), each
 * padded to 256 bytes, then stage 1's batch exactly as K14 sizes it (sd_rank_depth_rows_per_batch of what is left).
 * sd_extremal_workspace_bytes recommends a size, sd_extremal_min_workspace_bytes is the floor (one row per batch); both
 * are 0 for a shape or algo the call refuses.  The integers do not depend on the workspace size.
 * targets: m int64 indices of sample curves (device), NULL = all (m == n).  out: m int64 (device).
 * SD_ERR_INVALID for NULL X or out, T < 1, n < 2 or an unknown algo; SD_ERR_UNSUPPORTED for T > 16 384, for 2^31 or more
 * curves, for algo = 1 with n > 16 384, or where the worst-case walk n m T exceeds 10^14 entry comparisons;
 * SD_ERR_WORKSPACE below the floor.  All before any device work.  Every launch is bounded in work. */
size_t sd_extremal_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int algo);
size_t sd_extremal_min_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int algo);
int sd_extremal_counts(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const int64_t *targets, int64_t m,
                       int algo, int64_t *out, void *ws, size_t ws_bytes, void *stream);

/* ---- K16: central regions, fence, outside counts and whiskers of the functional boxplot ----
 * (Sun & Genton, JCGS 2011, from the modified band depth; Narisetty & Nair 2016 from the extremal depth.)  No reference
 * code.  X is T x n fp64 in either layout, finite or +-inf; NaN is NOT supported (the host layer refuses it).
 * Levels.  level: n bytes (device), level[i] in 0 .. L, 1 <= L <= 8.  Region l is { i : level[i] <= l }, l = 0 .. L - 1,
 * so regions are nested; level[i] >= L means "in no region".  The host derives the bytes from a depth vector and ascending
 * fractions alphas[0 .. L): curves ranked by descending depth (ties: the earlier column is deeper), region l the first
 * min(n, max(1, ceil(alphas[l] n))) of them, level[i] the smallest l whose region holds i.
 * Every output is an input value, an integer, or one of four rounded fp64 operations:
 *   env[l][0][t] = min, env[l][1][t] = max of X[t][i] over region l            (+inf / -inf for an empty region);
 *   fence of the region `box` with the factor F >= 0, per t, each line ONE rounded operation (no contraction):
 *       r = upper - lower;  w = F * r;  lf = lower - w;  uf = upper + w;     fence[0][t] = lf, fence[1][t] = uf
 *     (plain IEEE: a row whose box region is all +inf has a NaN fence, and a NaN fence flags nobody);
 *   outside[i][0] = #{ t : X[t][i] < lf[t] },  outside[i][1] = #{ t : X[t][i] > uf[t] }   (int32; a curve is an outlier
 *     iff either is nonzero; a member of the box region never is);
 *   whisker[0][t] / whisker[1][t] = min / max of X[t][i] over the curves that are not outliers.
 * The sign of a zero among equal values is not specified.
 * Example: rows [1,2,3,4,9], [2,2,2,2,-7], [0,5,1,3,2] (T = 3, n = 5), level = [1,0,0,1,2], L = 2, box = 0, F = 1.5:
 *   env[0] = (2,2,1) .. (3,2,5), env[1] = (1,2,0) .. (4,2,5), fence = (0.5,2,-5) .. (4.5,2,11),
 *   outside = [0 0; 0 0; 0 0; 0 0; 1 1] (9 > 4.5, -7 < 2), whisker = (1,2,0) .. (4,2,5).
 * Routes.  Up to sd_central_regions_row_capacity() (16 384) curves a workgroup holds whole rows in registers: per row and
 * exact level the min / max are reduced over the thread, the wave and the workgroup, one thread accumulates the levels,
 * writes env and the fence, the fence goes back through LDS and every thread compares the values it still holds; the
 * counts stay in registers over the workgroup's rows and meet in integer atomic adds (exact in any order), so X is read
 * once for regions, fence and counts.  Above the capacity, for any n < 2^31: blocks of 8192 curves write their min / max per
 * (row, level) to the workspace, a second kernel folds them into env and the fence, a third reads X again for the counts.
 * The whiskers are a further launch of the envelope code with one level, outside == (0, 0).  Dependencies between passes
 * are kernel boundaries; every loop is bounded by T or n.  A curve-major X takes a time-major copy first.
 * Workspace, in this order, each padded to 256 bytes: the time-major copy of a curve-major X (8 T n bytes), a fence
 * (16 T), the counts (8 n: used where whisker is asked for without outside), and above the capacity the blocks' min / max
 * (16 T L ceil(n / 8192)).  sd_central_regions_workspace_bytes is the size the call needs (0 for a shape or L it refuses).
 * box = -1: envelopes only; fence, outside and whisker must be NULL.  box in [0, L): any of the three may be NULL.
 * env: L x 2 x T doubles; fence, whisker: 2 x T doubles; outside: n x 2 int32 (all device).
 * SD_ERR_INVALID for NULL X, level or env, T < 1, n < 1, strides that are neither layout, L outside [1, 8], box outside
 * [-1, L), a negative, NaN or infinite factor, or fence / outside / whisker with box = -1; SD_ERR_UNSUPPORTED for 2^31 or
 * more curves or timepoints; SD_ERR_WORKSPACE when ws_bytes is below sd_central_regions_workspace_bytes.  All before any
 * device work. */
int64_t sd_central_regions_row_capacity(void);
size_t sd_central_regions_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int L);
int sd_central_regions(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const uint8_t *level, int L, int box,
                       double factor, double *env, double *fence, int32_t *outside, double *whisker, void *ws, size_t ws_bytes,
                       void *stream);

/* ---- K17: total variation depth and modified shape similarity of curves (Huang & Sun 2019) ----
 * No reference code.  X is T x n fp64 in either layout; NaN is NOT supported (the host layer refuses it).  Infinities are
 * ranked like any value; they make SN and SW non-finite under IEEE rules (the host layer refuses them for 'mss').
 * For a target q the whole sample counts, q included:
 *   a_t = #{j : X[t][j] <= X[t][q]}                                   (n - A of K14: 1 <= a_t <= n);
 *   c_t = #{j : X[s][j] <= X[s][q] and X[t][j] <= X[t][q]},  s = t - 1, for t >= 1.
 * Total variation depth: TVD(q) = (1/T) sum_{t=0..T-1} a_t (n - a_t) / n^2, at most 1/4.  The device returns the integer
 *   SD = sum_t a_t (n - a_t)  (<= T n^2 / 4, fits int64) and the host forms SD / (n^2 T) with one fp64 division.
 * Shape similarity at step t >= 1:  S_t = (n c_t - a_s a_t)^2 / (a_s (n - a_s) a_t (n - a_t)), the squared phi coefficient
 *   of the 2 x 2 table of the indicators at s and t; it equals Var(E[R_t | R_s]) / Var(R_t) of the paper and lies in [0, 1].
 *   Where the denominator is 0 (a_s = n or a_t = n) the numerator is 0 as well and S_t = 1: our convention.
 *   In fp64: e = (double)(n c_t - a_s a_t), exact since |e| <= n^2 < 2^53, then
 *   S_t = (e * e) / ((double)(a_s (n - a_s)) * (double)(a_t (n - a_t))), the integer products formed in 64-bit integers:
 *   three rounded operations.
 * Modified shape similarity: MSS(q) = sum_{t>=1} v_t S_t, v_t = |X[t][q] - X[t-1][q]| / sum_{u>=1} |X[u][q] - X[u-1][q]|.
 *   The device returns three doubles per target, SS = sum S_t, SN = sum |D_t| S_t, SW = sum |D_t|; the host returns SN / SW
 *   when SW > 0 and SS / (T - 1) for a constant curve.  MSS = 1 for a family of parallel curves.
 * Example: rows [1,2,2,4], [2,1,3,3], [1,3,2,4] (T = 3, n = 4): a = (1,3,3,4), (2,1,4,4), (1,3,2,4); c = (1,1,3,4), (1,1,2,4);
 *   SD = [10, 9, 7, 0]; S_1 = (1/3, 1/9, 1, 1), S_2 = (1/3, 1/9, 1, 1).
 * Routes: algo 1, n <= 16 384: K14's pair image (B | A << 16 per row and curve), then one workgroup per pair of consecutive
 *   rows counts c of all n curves in LDS -- a weak 2-D dominance count of the points (B(s), B(t)): a counting scatter per
 *   row, a block histogram over strips of 128 positions with a 2-D prefix sum, two strip scans per curve -- and stores c - 1
 *   as u16; a fold with one owner per (target, row slice) forms the sums.  algo 2, any n < 2^31: a pairwise kernel over the
 *   doubles alone counts a_s, a_t and c_t by comparison, O(T n m) (SD_ERR_UNSUPPORTED above 10^14 comparisons), and feeds
 *   the same arithmetic.  algo 0 (auto): algo 1 up to 16 384 curves, algo 2 above.
 * Workspace, in this order, each padded to 256 bytes: the time-major copy of a curve-major X (8 T n bytes), the row slices'
 * records (512 m), and on algo 1 the last image row of the batch before (4 n), c - 1 of a batch (2 n per row) and stage 1's
 * batch as K14 sizes it.  sd_tvd_workspace_bytes recommends a size, sd_tvd_min_workspace_bytes is the floor (one row per
 * batch), sd_tvd_rows_per_batch says how many rows a batch of a call with ws_bytes takes (T on algo 2); all are 0 for a shape
 * or algo the call refuses or below the floor.  A pair of rows straddles every batch boundary; each pair is counted exactly
 * once, and neither the integers nor the doubles depend on the workspace size.
 * targets: m int64 curve indices (device), NULL = all (m == n).  sd_sum: m int64.  shape: m x 3 doubles (SS, SN, SW).
 * counts: NULL, or (T - 1) x m uint32, counts[t - 1][q] = c_t of target q (all device).  T = 1 gives SD only: shape is
 * zeroed and counts is untouched.
 * SD_ERR_INVALID for NULL X, sd_sum or shape, T < 1, n < 1 or an unknown algo; SD_ERR_UNSUPPORTED for n < 2, for algo = 1
 * with n > 16 384, or for 2^31 or more curves or timepoints; SD_ERR_WORKSPACE below the floor.  All before any device work. */
size_t sd_tvd_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int algo);
size_t sd_tvd_min_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int algo);
int64_t sd_tvd_rows_per_batch(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int algo, size_t ws_bytes);
int sd_tvd_sums(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const int64_t *targets, int64_t m, int algo,
                int64_t *sd_sum, double *shape, uint32_t *counts, void *ws, size_t ws_bytes, void *stream);

/* ---- K18: halfspace and projection depth of multivariate curves, integrated over time ----------
 * No reference code (the multivariate functional halfspace depth of Claeskens, Hubert, Slaets & Vakili 2014 and its
 * projection-depth sibling, over a fixed direction set).  P is n x T x d row-major fp64, P[i][t][e] (device), d <= 8; U is
 * k x d row-major (device), shared by all timepoints.  The cloud at t is C_t = {P[i][t][:]}: n points, the target among them.
 *   h_t(i) = K10's count of point i in C_t (min over the directions of min(ge, le), the point and every tie counted);
 *   O_t(i) = K12's outlyingness of point i in C_t (median rule, MAD without factor, one correctly rounded division, a
 *            numerator of 0 gives 0, a positive one with MAD = 0 gives +inf);
 * both on K10's projection bits.  The records per target:
 *   sd_multi_halfspace_sums:   out[q] = (SH, MH) = (sum_t h_t, min_t h_t), int64.  Host: mean depth = SH / (n T), infimal
 *                              depth = MH / n.
 *   sd_multi_projection_sums:  out[q] = (PS, OM) = (sum_t 1 / (1 + O_t), max_t O_t), doubles.  A term of PS is one rounded
 *                              addition and one correctly rounded division (O = inf: 0.0); the terms are added in ascending
 *                              t from 0.0, one rounded addition per timepoint (the order of np.cumsum).  Host: mean depth =
 *                              PS / T, infimal depth = 1 / (1 + OM).
 * A numpy restatement gives the same bits, and nothing depends on algo, on the workspace size or on how directions and
 * timepoints are split: integer min and sum and the maximum of non-negative doubles are order-free, and PS is added by one
 * owner per target in ascending t, carried across the batches of timepoints in stream order.
 * Routes: algo 1 (lds), n <= sd_multi_cloud_lds_capacity() = 8192: a batch of timepoints is copied feature-major into the
 *   workspace; one workgroup per (timepoint, 32 directions) projects the cloud, sorts the n keys in its LDS (64 KB) and
 *   ranks every point in them (halfspace: a lower and an upper bound per point; projection: K12's selection of the median
 *   and the MAD); slices of a timepoint meet through atomicMin / atomicMax on the bit pattern.  algo 2 (global), any n: per
 *   timepoint the cloud is gathered and sd_halfspace_counts' / sd_projection_outlyingness' own launchers run on it.
 *   algo 0 (auto): algo 1 up to the capacity, algo 2 above.
 * Workspace: algo 1 holds per timepoint of a batch the copy (8 n d bytes) and every curve's value (4 n or 8 n); algo 2 the
 * cloud (8 n d), the values (8 n) and K10's / K12's workspace.  sd_multi_*_workspace_bytes recommends a size,
 * sd_multi_*_min_workspace_bytes is the floor (one timepoint per batch; one direction per chunk); both are 0 for a shape or
 * algo the call refuses.
 * targets: m int64 curve indices (device), NULL = all (m == n); repeated and permuted entries are allowed; every curve is
 * ranked whatever m is.
 * SD_ERR_INVALID for NULL pointers, n, T, d, k < 1 or an unknown algo; SD_ERR_UNSUPPORTED for d > 8, 2^31 or more curves,
 * more than 10^14 projections and comparisons (T k n (d + log2 n)), or algo 1 above the capacity; SD_ERR_WORKSPACE below the
 * floor.  All before any device work.  Every launch is bounded in work. */
int64_t sd_multi_cloud_lds_capacity(void);
size_t sd_multi_halfspace_workspace_bytes(int64_t n, int64_t T, int d, int64_t k, int64_t m, int algo);
size_t sd_multi_halfspace_min_workspace_bytes(int64_t n, int64_t T, int d, int64_t k, int64_t m, int algo);
int sd_multi_halfspace_sums(const double *P, int64_t n, int64_t T, int d, const double *U, int64_t k, const int64_t *targets,
                            int64_t m, int algo, int64_t *out, void *ws, size_t ws_bytes, void *stream);
size_t sd_multi_projection_workspace_bytes(int64_t n, int64_t T, int d, int64_t k, int64_t m, int algo);
size_t sd_multi_projection_min_workspace_bytes(int64_t n, int64_t T, int d, int64_t k, int64_t m, int algo);
int sd_multi_projection_sums(const double *P, int64_t n, int64_t T, int d, const double *U, int64_t k, const int64_t *targets,
                             int64_t m, int algo, double *out, void *ws, size_t ws_bytes, void *stream);

/* ---- K19: directional outlyingness of multivariate curves (the records of the MS-plot) ---------
 * No reference code (Dai & Genton 2018, 2019: the Stahel-Donoho outlyingness with a direction; its mean over time shows a
 * magnitude outlier, its variation over time a shape outlier).  P, U, targets, algo as for K18.  Per timepoint t:
 *   o_t(i) = K18's O_t(i), on the same bits;
 *   c_t    = the LOWEST curve index among those minimising o_t over ALL n curves (whatever the targets are): the sample point
 *            of largest projection depth, the median of the cloud over the direction set;
 *   diff_e = P[i][t][e] - P[c_t][t][e];  s = sum_e diff_e^2, added in ascending e, each term one rounded multiplication and
 *            one rounded addition (no fma);  r = sqrt(s), correctly rounded;
 *   O_t(i)_e = o_t(i) * (diff_e / r): one rounded division and one rounded multiplication.
 *   r == 0: O_t(i) is the zero vector -- the centre itself, its duplicates, and differences so small that their squares
 *            underflow.  o_t(i) = +inf (a direction's MAD is 0) is NOT special-cased: the products follow IEEE, +-inf, or NaN
 *            where diff_e = 0.
 * Per target, over ascending t, a Welford record of d running means M_e and one running sum Q, both from 0.0: at timepoint
 * t, with c = (double)(t + 1), for e ascending
 *   delta_e = O_e - M_e;   M_e = M_e + delta_e / c;   Q = Q + delta_e * (O_e - M_e(new))       every operation rounded once.
 * out[q] = (M_0 .. M_(d-1), Q), d + 1 doubles.  Host: MO = M, VO = Q / T, FO = sum_e M_e^2 + VO.
 * centres (NULL or T int64, device): c_t.  curves (NULL or m x T x d doubles, device): O_t of every target; both cost nothing
 * when NULL, and neither is written when m == 0.
 * A numpy restatement gives the same bits, and nothing depends on algo, on the workspace size or on how directions and
 * timepoints are split: o_t is order-free, c_t is an argmin with a fixed tie rule, and the record has one owner per target
 * in ascending t, carried in out[] across the batches of timepoints in stream order.
 * The project-sort-select stage is K18's, launch for launch; per batch of timepoints one workgroup per timepoint then
 * reduces every curve's value to c_t, and a thread per target folds the batch into its record.
 * Workspace: sd_multi_projection_*'s layout plus 8 bytes per timepoint of a batch (the centres, padded to 256 bytes as a
 * whole); recommended size, floor and the value 0 as for K18.
 * The refusals are sd_multi_projection_sums', in its order, all before any device work.  Every launch is bounded in work. */
size_t sd_multi_outlyingness_workspace_bytes(int64_t n, int64_t T, int d, int64_t k, int64_t m, int algo);
size_t sd_multi_outlyingness_min_workspace_bytes(int64_t n, int64_t T, int d, int64_t k, int64_t m, int algo);
int sd_multi_outlyingness_moments(const double *P, int64_t n, int64_t T, int d, const double *U, int64_t k,
                                  const int64_t *targets, int64_t m, int algo, double *out, int64_t *centres, double *curves,
                                  void *ws, size_t ws_bytes, void *stream);

/* ---- K20: squared L2 distances between curves, their k-th smallest, and the h-modal sums --------
 * No reference code (the h-modal depth of Cuevas, Febrero & Fraiman 2006, depth.mode of fda.usc, and its substrate, the
 * matrix of pairwise L2 distances).  X, T, n, st, sn as for sd_rank_depth_sums; the values are finite with |x| <= 2^480 (the
 * caller checks; nothing then overflows for T < 2^31).  A target is a sample curve (targets: m int64 indices on the device,
 * NULL = all, m == n; repeated and permuted entries are allowed) or, in the external forms, column q of Q (T x m, time-major
 * dense, device, as in sd_mbd_external_counts).
 * Squared distance of target x and sample curve j: one accumulator over ascending t from +0.0,
 *   d = x[t] - X[t][j];   acc = fma(d, d, acc)                            two rounded operations per timepoint,
 * never split over t, no Gram form, no matrix instructions.  So D2[i][j] and D2[j][i] hold the same bits, D2[i][i] = +0.0, and
 * a subnormal product is kept.  The L2 distance is sqrt(D2); the library returns D2.
 *   sd_curve_sqdist, sd_curve_sqdist_external:  out[q * n + j] = D2 of target q and sample curve j, m x n doubles.
 *   sd_curve_sqdist_select:  out[0] = the k-th smallest (k 1-based, 1 <= k <= N = n (n - 1) / 2) of D2[i][j] over the pairs
 *     i < j: a radix descent on the 64-bit images (nonnegative doubles order like them), digits of 11 bits from the top,
 *     integer histograms in LDS and global memory, the digit of rank k picked on the device.  With room for the n x n matrix
 *     in the workspace (at most 1 GiB) it is formed once and re-read per pass, otherwise every pass recomputes it; the result
 *     is the same.
 *   sd_hmodal_sums, sd_hmodal_external_sums:  out[q] = S = sum_j exp(-(D2[q][j] * g)) over all n sample curves (for a sample
 *     target its own term, exactly 1.0, included); g = 1 / (2 h^2) is the caller's double.  The product is rounded once, exp
 *     is the device math library's (within 1 ulp).  The terms are added in an order that depends on n alone (written out in
 *     csrc/curve_dist.hip: tiles of 64 sample curves, inside a tile 16 lanes of 4 columns joined by a butterfly, the tiles
 *     in ascending order), without floating-point atomics: S of a target holds the same bits whatever the target list, the
 *     layout of X or the workspace size.
 * One tile kernel serves all five: a workgroup per 128 targets x 64 sample curves, both panels staged in LDS 16 timepoints
 * at a time, an 8 x 4 register tile per thread, and the epilogue (store, exp-and-add, histogram) chosen at compile time.
 * Workspace, each part padded to 256 bytes: the time-major copy of a curve-major X (8 T n bytes); then for `what` =
 *   0 (distances): nothing;   1 (h-modal sums): the tiles' partial sums of a batch of targets, 8 ceil(n / 64) bytes a target,
 *   batches of whole blocks of 128 targets (the floor is one block; the recommended size holds all, up to 256 MiB);
 *   2 (selection): histogram and state (16 640 bytes: the floor), then the n x n matrix where it is at most 1 GiB.
 * sd_curve_sqdist_workspace_bytes recommends a size, sd_curve_sqdist_min_workspace_bytes is the floor (both may be 0: a
 * time-major X and what = 0 need no workspace, and ws may then be NULL), sd_curve_sqdist_targets_per_batch says how many
 * targets a batch of a call with ws_bytes takes (0 below the floor; all m for what = 0, all n for what = 2).  All three are 0
 * for a shape or `what` the calls refuse.
 * SD_ERR_INVALID for NULL X, Q or out, T < 1, n < 1, m < 0, k outside [1, N], g not positive and finite; SD_ERR_UNSUPPORTED for
 * n < 2, for 2^31 or more curves or timepoints, or for more than 10^14 pair-timepoints (n m T; the selection counts 3 n^2 T);
 * SD_ERR_WORKSPACE below the floor.  All before any device work.  Every launch is bounded in work. */
size_t sd_curve_sqdist_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int what);
size_t sd_curve_sqdist_min_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int what);
int64_t sd_curve_sqdist_targets_per_batch(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int what, size_t ws_bytes);
int sd_curve_sqdist(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const int64_t *targets, int64_t m, double *out,
                    void *ws, size_t ws_bytes, void *stream);
int sd_curve_sqdist_external(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const double *Q, int64_t m, double *out,
                             void *ws, size_t ws_bytes, void *stream);
int sd_curve_sqdist_select(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, int64_t k, double *out, void *ws,
                           size_t ws_bytes, void *stream);
int sd_hmodal_sums(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const int64_t *targets, int64_t m, double g,
                   double *out, void *ws, size_t ws_bytes, void *stream);
int sd_hmodal_external_sums(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const double *Q, int64_t m, double g,
                            double *out, void *ws, size_t ws_bytes, void *stream);

/* ---- K21: the functional spatial depth of curves -------------------------------------------------
 * No reference code (Chakraborty & Chaudhuri 2014; Sguera, Galeano & Lillo 2014; depth.FSD of fda.usc):
 *   FSD(x) = 1 - | (1/N) sum_j (x - x_j) / |x - x_j| |,  L2 norms over the time grid (uniform: the quadrature weight cancels, so
 * this is the Euclidean spatial depth in R^T).  X, T, n, st, sn, the values' contract (finite, |x| <= 2^480), targets and Q as
 * for K20.  Per target x, with Y the time-major X:
 *   1. D2[j] = K20's squared distance on K20's bits: one accumulator over ascending t from +0.0, d = x[t] - Y[t][j];
 *      acc = fma(d, d, acc).
 *   2. w[j] = 0.0 where D2[j] == 0.0, else 1.0 / sqrt(D2[j]): a correctly rounded root, then one correctly rounded division.
 *   3. A coincident curve (D2 == 0: the target's own column, a duplicate of it, or differences so small that every square
 *      underflows inside the fma) adds nothing to the sum and still counts in the sample size: the papers' sum over
 *      x_j != x.  K5 (sd_l1_depth) returns NaN for coincident points because its reference does; K21 differs on purpose.  No
 *      target index is special-cased: repeated and permuted target lists work, and so do external targets equal to a sample
 *      curve.
 *   4. E[t], per timepoint one accumulator over ascending j = 0 .. n - 1 from +0.0: d = x[t] - Y[t][j]; E = fma(w[j], d, E).
 *      The direct form, never split over j, no Gram form x sum w - sum w_j x_j (it cancels for curves that are close relative
 *      to their level), no matrix instructions, no floating-point atomics: E holds the same bits whatever the target list,
 *      the tiles, the layout of X or the workspace.
 *   5. S, one accumulator over ascending t from +0.0: S = fma(E[t], E[t], S).
 *   out[q] = S (m doubles);  field = NULL, or m x T doubles, target-major, that receive E (at no cost when NULL).
 *   6. The caller forms depth = 1 - sqrt(S) / N, N = n for a sample target and n + 1 for an external one (K5's convention: the
 *      sample the depth refers to includes the target).
 * D2 < 2^993, w >= 2^-497, |E| <= about n, S <= about n^2: nothing overflows under the values' contract.
 * Three kernels per batch of targets: K20's tile kernel with a fourth epilogue that stores w (csrc/curve_dist.hip); the sum
 * kernel, a workgroup per 128 targets x 64 timepoints (x 32 where that leaves compute units idle) that walks all n sample
 * curves in ascending order, 16 at a time through LDS, an 8 x 4 (8 x 2) register tile of accumulators and of the targets' own
 * values per thread (csrc/spatial_depth.hip); and the fold, one thread per target.
 * Workspace, each part padded to 256 bytes: the time-major copy of a curve-major X (8 T n bytes); the weights of a batch of
 * targets, 8 n bytes a target; the field of a batch, 8 T bytes a target (with `field` given the kernel writes there instead).
 * Batches are whole blocks of 128 targets; the floor is one block.  The recommended size holds all targets, up to 8 GiB of
 * weights a batch: at 100 000 curves x 256 timepoints that is 83 blocks, 664 workgroups of the sum kernel, more than two for
 * each of the 256 compute units, where 1 GiB would give 80.  sd_spatial_targets_per_batch says how many targets a batch of a
 * call with ws_bytes takes (0 below the floor).  All three are 0 where T < 1, n < 2, m < 0 or T or n is 2^31 or more (what the
 * calls refuse for another reason, the budget of pair-timepoints among it, still has its sizes); the floor is 0 for m == 0.
 * sd_spatial_time_tile says which time tile the sum kernel takes for a batch of `targets` targets on the stream's device: 64,
 * or 32 where the 128 x 64 tile would give fewer than two workgroups per compute unit (0 for T < 1 or targets < 1).  The
 * results do not depend on it.
 * The refusals are K20's, in K20's order, all before any device work: SD_ERR_INVALID for NULL X, Q or out, T < 1, n < 1, m < 0;
 * SD_ERR_UNSUPPORTED for n < 2, for 2^31 or more curves or timepoints, or for more than 10^14 pair-timepoints (2 n m T: the two
 * passes); SD_ERR_WORKSPACE below the floor.  Every launch is bounded in work; no workgroup waits for another. */
size_t sd_spatial_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m);
size_t sd_spatial_min_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m);
int64_t sd_spatial_targets_per_batch(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, size_t ws_bytes);
int64_t sd_spatial_time_tile(int64_t T, int64_t targets, void *stream);
int sd_spatial_sums(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const int64_t *targets, int64_t m, double *out,
                    double *field, void *ws, size_t ws_bytes, void *stream);
int sd_spatial_external_sums(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const double *Q, int64_t m, double *out,
                             double *field, void *ws, size_t ws_bytes, void *stream);

/* ---- K22: the lens, spherical and beta-skeleton depth of curves and point clouds -----------------
 * No reference code (lens depth: Liu & Modarres 2011, Kleindessner & von Luxburg 2017, Geenens, Nieto-Reyes & Francisci 2023;
 * spherical depth: Elmore, Hettmansperger & Xuan 2006; beta-skeleton depth: Yang & Modarres 2018).  The depth of x is the share
 * of the pairs (x_i, x_j), i < j, of the sample whose beta-lune holds x.  It needs nothing of the data but distances, so X (T x n,
 * st, sn, values, targets and Q as for K20) is as well a cloud of n points in R^T, any T >= 1.
 * With D2 K20's squared distance on K20's bits (symmetric, +0.0 diagonal), a = D2(x, x_i), b = D2(x, x_j), c = D2(x_i, x_j) and
 * kappa = 2 / beta - 1 in [-1, 1] (beta in [1, inf]; beta = 2: the lens, kappa = 0; beta = 1: the sphere, kappa = 1), x lies in
 * the lune iff  a + kappa b <= c  and  b + kappa a <= c  (from |l u + (1 - l) v|^2 = l |u|^2 + (1 - l) |v|^2 - l (1 - l) |u - v|^2
 * with l = beta / 2).  The device evaluates exactly
 *   t1 = kappa * b;  s1 = a + t1;  t2 = kappa * a;  s2 = b + t2;  in = (s1 <= c) && (s2 <= c)
 * with four separately rounded operations (no fused multiply-add), and
 *   out[q] = G = #{i < j : in}  (m int64);  the caller forms depth = G / C(n, 2), for a sample and for an external target alike.
 * Three compile-time forms give the same integers where they overlap: kappa == 0.0: a <= c && b <= c; kappa == 1.0:
 * (a + b rounded) <= c, one test; and the general form, any kappa.  algo = 0 picks the form by kappa, algo = 1 forces the general
 * form (the cross-check).  No index is special-cased: a sample target's own pairs (a = 0, c = b) satisfy the predicate and
 * count, as in the papers' sum over all pairs; coincident curves (c = 0) count only for a coincident target (at kappa = -1, beta
 * = inf, for every target: the slab between two equal hyperplanes is read as the whole space); repeated and
 * permuted target lists work, and so do external targets equal to a sample curve, which get that curve's count.  D2 < 2^993,
 * so nothing overflows.  On data whose right angles are exact in the reals but whose values are not representable (rounded to
 * 0.1, say) the spherical count follows the rounded D2, not the real geometry; on integer-valued data of small magnitude D2
 * is exact and the counts are the geometric ones.
 * Stage 1 forms the whole n x n matrix through K20's tile kernel (and, for external targets, the m x n rows of a batch); a
 * sample target's row is read from the matrix through the target list.  Stage 2 counts: a workgroup per 128 targets x 64
 * sample curves i x a span of tiles of 64 sample curves j at or above the diagonal, an 8 x 4 register tile of a per thread, c
 * and the targets' b staged in LDS 16 j at a time, 32-bit counters per lane, one integer atomic per target and workgroup
 * (csrc/lens_depth.hip).  The counts are integers: they do not depend on the tiles, the target list, the layout of X or the
 * workspace size.
 * Workspace, each part padded to 256 bytes: the time-major copy of a curve-major X (8 T n bytes); the matrix, 8 n^2 bytes; the
 * rows of a batch of external targets, 8 n bytes a target, whole blocks of 128 (the floor is one block; the recommended size
 * holds all m, up to 1 GiB).  Both calls take the same sizes; sample targets use no rows and always go in one batch.
 * sd_lens_targets_per_batch says how many external targets a batch of a call with ws_bytes takes (0 below the floor).  All
 * three are 0 for a shape the calls refuse on shape; the floor is 0 for m == 0.
 * The refusals, all before any device work: SD_ERR_INVALID for NULL X, Q or out, T < 1, n < 1, m < 0, kappa NaN or outside
 * [-1, 1], algo outside {0, 1}; SD_ERR_UNSUPPORTED for n < 2, for n > 16 384 (the stored matrix is 2 GiB there and no route
 * recomputes it), for 2^31 or more timepoints, or for more than 10^14 pair-timepoints (n (n + m) T); SD_ERR_WORKSPACE below
 * the floor.  Every launch is bounded in work; no workgroup waits for another. */
size_t sd_lens_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m);
size_t sd_lens_min_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m);
int64_t sd_lens_targets_per_batch(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, size_t ws_bytes);
int sd_lens_counts(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const int64_t *targets, int64_t m, double kappa,
                   int algo, int64_t *out, void *ws, size_t ws_bytes, void *stream);
int sd_lens_external_counts(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const double *Q, int64_t m, double kappa,
                            int algo, int64_t *out, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* STATDEPTH_HIP_H */
