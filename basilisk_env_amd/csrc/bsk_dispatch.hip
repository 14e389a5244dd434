// bsk_dispatch.hip — the step kernel's instantiations live in eight translation units (bsk_kernels.hip compiled with -DBSK_TU=0..7:
// about one minute with make -j instead of six in one unit); this is the dispatcher that tries them in turn.
#include "bsk_launch.hpp"

namespace bsk {

#define BSK_UNITS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
#define DECL(k) hipError_t dispatch_step_tu##k(int, int, bool, int, int, int, int, const StepLaunch*, KernelDesc*);
BSK_UNITS(DECL)
#undef DECL

// (a cell lives in one unit: the one that describes the kernel has also launched it, if asked to)
hipError_t dispatch_step(int grav, int nrw, bool diag, int feat, int form, int block, int n, const StepLaunch* go, KernelDesc* d) {
    hipError_t e;
#define TRY(k) e = dispatch_step_tu##k(grav, nrw, diag, feat, form, block, n, go, d); if (d->fn) return e;
    BSK_UNITS(TRY)
#undef TRY
    return hipErrorInvalidValue;
}

}  // namespace bsk
