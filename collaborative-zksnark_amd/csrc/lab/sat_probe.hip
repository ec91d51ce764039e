// sat_probe.hip -- LAB BUILD ONLY (build.py LAB_SOURCES, with -DCZK_NOINLINE_MUL): the saturated field.h / tower.h / curve.h probes in the form
// pairing.hip, point_codec.hip, msm.hip, lanes.hip, net.hip and net_rounds.hip are built with -- the Montgomery multiply a real function.  The same
// probes with the multiply inlined are compiled in arith_probe.hip, whose czk_lab_arith_probe dispatches here.
#ifndef CZK_NOINLINE_MUL
#error "sat_probe.hip is the -DCZK_NOINLINE_MUL form of the probes"
#endif
#include "arith_probe.h"

#include "curve.h"
#include "czk_internal.h"
#include "tower.h"

namespace czk {
namespace {
#include "sat_probe.h"
}  // namespace

int sat_probe_noinline(czk_ctx* ctx, int fn, const uint32_t* in, size_t iw, uint32_t* out, size_t ow, size_t n, int mem) {
    return sat_probe_dispatch(ctx, fn, in, iw, out, ow, n, mem);
}
}  // namespace czk
