// xcheck.hip -- the one translation unit that is compiled twice: where the cross-check build differs from the product.
//
// libstatdepth_hip.so (the product) gets this file WITHOUT -DSD_CROSSCHECK: xswitch() is the constant 0, no environment
// variable can select another implementation, and the hooks to the retired kernel generations (rank_routes.h; K4's in
// sd_common.h) fail -- nothing calls them, and the retired generations are not in the binary.
// libstatdepth_hip_xcheck.so (loaded only by tests/) gets it with -DSD_CROSSCHECK: xswitch() reads the environment per
// call, and the hooks are defined next to the retired kernels in translation units of that library alone
// (mbd_rank.hip, mbd_rank_ab_retired.hip, mbd_rank_big_retired.hip, simplex_retired.hip): independent implementations
// the parity tests compare the product path with.  Every other object file is the same one in both libraries.
#include <stdlib.h>

#include "sd_common.h"
#include "rank_routes.h"

namespace sd {

#ifdef SD_CROSSCHECK
long long xswitch(const char *name) {
    const char *e = getenv(name);
    return e ? atoll(e) : 0;
}
#else
long long xswitch(const char *) { return 0; }

int retired_rank_sorts(const double *, i64, i64, i64, u32 *, u32 *, int, hipStream_t) {
    return fail(SD_ERR_UNSUPPORTED, "sort-based rank kernels exist in cross-check builds only");
}
int retired_rank_v1(const double *, i64, i64, const i64 *, i64, i64, int, u64 *, void *, size_t, hipStream_t) {
    return fail(SD_ERR_UNSUPPORTED, "rank implementation 1 exists in cross-check builds only");
}
int retired_big_rank_batch(const BigBatch &, hipStream_t, const u32 **) {
    return fail(SD_ERR_UNSUPPORTED, "retired large-n rank generations exist in cross-check builds only");
}
int retired_simplex_generic(const double *, i64, i64, int, const PointSel &, int, double, u64, u64, i64, u64, i64, u64 *, dim3,
                            hipStream_t) {
    return fail(SD_ERR_UNSUPPORTED, "the generic simplex kernel exists in cross-check builds only");
}
#endif

}  // namespace sd

extern "C" int sd_is_crosscheck_build(void) {
#ifdef SD_CROSSCHECK
    return 1;
#else
    return 0;
#endif
}
