// The production builds of kron_v5_kernel at p = 2 (kron_v5_kernel.hpp: kV5Production).
#include "common.hpp"
#include "kron_v5_kernel.hpp"
#include "launchers.hpp"
#include "wave_ops.hpp"   // (every header named here: the build's dependency scan reads this file only)

namespace poms {

#ifndef POMS_V5_QUICK   // (POMS_V5_QUICK: p = 3 production builds only, for quick tuning builds)
int kron_v5_launch_p2(int epi, int store, const V5Launch& a) { return v5_launch_production<2>(epi, store, a); }
#endif

}  // namespace poms
