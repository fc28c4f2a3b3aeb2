// strict_routes.h -- what the translation units of the strict band depth (bd_strict.hip, bd_strict_class.hip,
// bd_strict_subsets.hip, bd_strict_grid.hip) call in each other: the shape predicates of the routes, the route plan of one
// call, and the launchers behind it (internal; what sd_api.hip dispatches to is in sd_common.h).  Included by rank_routes.h.
#pragma once
#include "sd_common.h"

namespace sd {

constexpr int ST_THREADS = 256;

// ---- bd_strict_grid.hip: two to four coordinates at large n through a grid of cells instead of every pair of points ----
bool bd_strict_grid_applies(i64 T, i64 n, int J);
size_t bd_strict_grid_workspace_bytes(i64 T, i64 n, bool subset);
int launch_bd_strict_grid(const double *Y, i64 T, i64 n, const i64 *targets, i64 m, u64 *out, int jcols, u32 *flag, void *ws,
                          size_t ws_bytes, hipStream_t s);

// ---- which route takes a shape ----
// a series is "short" for the class kernel up to 5 timepoints: 81 / 243 counters per lane leave two to six waves per CU, and
// still O(n) per target beats masks + matching at every size (10^5 x 4: 21 against 755 ms; 10^4 x 5: 1.3 against 2.7 ms)
static inline bool strict_class_applies(i64 T, i64 n, int J) {
    (void)n;
    return J == 2 && T <= 5;
}
// 6 ... 8 timepoints: 729 ... 6 561 three-state classes per target are too many for a histogram per lane; a workgroup takes a
// few targets and counts into shared histograms (strict_class_wg_kernel).  NaN-free data only: four states would be 4^T
// counters (256 KB at T = 8), so data with NaN goes the way it went before (masks + matching up to 131 071 curves).
static inline bool strict_class_wg_applies(i64 T, int J) { return J == 2 && T >= 6 && T <= 8; }
// complement matching: the keys carry a 17-bit curve id
constexpr i64 ST_MATCH_MAXN = 131071;
static inline bool strict_match_applies(i64 T, i64 n, int J) { return J == 2 && (T + 31) / 32 <= 65535 && n <= ST_MATCH_MAXN; }
// Without matching every pair of curves is tested for every target (m n^2 / 2 pair tests at ~2e11 per second): what would
// keep the GPU for hours is refused instead of started
constexpr double ST_PAIR_TESTS_MAX = 2.0e14;
static inline double strict_pair_tests(i64 n, i64 m) { return (double)m * (double)n * (double)n * 0.5; }
static inline bool strict_pair_tests_refused(i64 n, i64 m) { return strict_pair_tests(n, m) > ST_PAIR_TESTS_MAX; }
// 6 ... 8 timepoints beyond the matching's reach, with more pairs than the pair kernel is allowed: the classes are the ONLY route
static inline bool strict_class_wg_only(i64 T, i64 n, i64 m, int J) {
    return strict_class_wg_applies(T, J) && n > ST_MATCH_MAXN && strict_pair_tests_refused(n, m);
}

// ---- the route plan of one call (bd_strict.hip: strict_plan) ----
// Every decision the size functions and the launchers take, made in one place from the shape and -- cross-check builds only --
// the SD_STRICT_* switches (the product's xswitch() is 0).  Computed per call: the tests change the environment between calls.
struct StrictPlan {
    bool classes;        // J = 2, T <= 5: state classes, the whole call (launch_bd_strict_classes) ...
    bool grid;           // ... two to four coordinates at large n, targets not a small subset: through the grid of cells
    bool laneclass;      // ... T = 3, 4, 5 without NaN: the histogram-per-lane kernel instead of the workgroup form
    bool class_wg;       // J = 2, 6 <= T <= 8: a NaN flag in front of the mask pipeline, NaN-free data through the workgroup form
    bool class_wg_only;  // ... and nothing behind it: data with NaN is refused (a property of the shape, whatever the switches)
    bool match;          // clean pairs by complement matching (else every pair is tested)
    bool rankmasks;      // masks from the 16-bit rank image (n <= 32 767)
    bool rank32;         // masks from the large-n route's 32-bit rank image (32 767 < n <= 131 071)
    bool gen2;           // second-generation mask and pair kernels (J = 2, T <= 1024)
    bool force_global;   // every target's groups through the global-memory table
    bool pairs2;         // every partner of a dirty curve through the mask test (strict_pairs2_kernel)
};
// external: the targets are not curves of Y (no rank image of theirs, no grid).  The size functions plan with external = false.
StrictPlan strict_plan(i64 T, i64 n, i64 m, int J, bool external);

// ---- bd_strict_class.hip: the state-class kernels ----
// flag[0] = 1 when Y (T x n) or the external targets Q (T x m; null: none) hold a NaN; flag[0] is zeroed by the caller
void launch_strict_any_nan(const double *Y, i64 T, i64 n, const double *Q, i64 m, u32 *flag, hipStream_t s);
// T <= 5, the whole call: the grid when the plan and the workspace allow it, else the lane / workgroup kernels
int launch_bd_strict_classes(const StrictPlan &plan, const double *Y, i64 T, i64 n, const i64 *targets, const double *Q, i64 m,
                             u64 *out, int jcols, void *ws, size_t ws_bytes, hipStream_t s);
// 3 <= T <= 8, NaN-free data: the workgroup form (nanflag: null, or the flag that makes it return at once)
int launch_bd_strict_class_wg(const double *Y, i64 T, i64 n, const i64 *targets, const double *Q, i64 m, const u32 *nanflag,
                              u64 *out, int jcols, hipStream_t s);

}  // namespace sd
