// The production builds of kron_v5_kernel at p = 3 (kron_v5_kernel.hpp: kV5Production).
#include "common.hpp"
#include "kron_v5_kernel.hpp"
#include "launchers.hpp"
#include "wave_ops.hpp"   // (every header named here: the build's dependency scan reads this file only)

namespace poms {

int kron_v5_launch_p3(int epi, int store, const V5Launch& a) { return v5_launch_production<3>(epi, store, a); }

}  // namespace poms
