// chk_w1bar.hip -- checker build only (lib/chk_w1bar, never the product library): sqp_rti_rowpar.hip with the block
// barrier at every phase boundary of the one-wave kernels, as before the team kernel's hand-off gave them the
// wave-local fence (W1Barrier, rowpar_layout.hpp). tests/test_gpu_team_handoff.py solves the same fleet with it and
// with the product and compares every output bit for bit.
#include "rowpar_layout.hpp"

namespace nmpc {
template <>
struct W1Barrier<void> {
    static constexpr bool value = true;
};
}  // namespace nmpc

#include "sqp_rti_rowpar.hip"
