// pnp_compile_prefix.h -- tests/test_pnp_solver_compiles.py: the stand-in declarations Tracking.cc is compiled against
// (oracle/ref_shim/tracking/tracking_stubs.h) declare a ygz::PnPsolver of their own, for a build in which PnPsolver stays outside.  The
// compile check of host/PnPsolver.cc wants everything else of that header and the product's class under the name: the stand-in gets another.
#define PnPsolver TrackingStubPnPsolver
#include "tracking_stubs.h"
#undef PnPsolver
#undef YGZ_PNPSOLVER_H_   // (the stand-in header claims the guard so that include/PnPsolver.h stays out; here the product's header takes it)
