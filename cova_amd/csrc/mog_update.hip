// The update kernels a MoG labeller in COVAHIP_MOG_SHADOWS_OFF runs: the SHADOW = false instances of all five kernels of
// mog_update.h, through the dispatch's.  Nothing else is in this file's object; the SHADOW = true instances are mog_shadow.hip's,
// and the two files build in parallel.
//
// No contraction in this file (see mog_dev.h): every product and sum is rounded on its own, as the x86 builds of OpenCV
// compute it, and the update kernels' ISA has no f32 fused multiply-add at all (DESIGN.md checks it).  It is built with the
// flags of mog.hip.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "covahip.h"
#include "internal.h"
#include "mog_dev.h"
#include "mog_update.h"

MOG_ROUTE_INSTANCE(false, false);
