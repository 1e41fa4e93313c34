// consensus_plan_harness.cc -- plan_wta_consensus (mgm_amd/csrc/mgm_planner.h) behind a C interface for
// tests/test_consensus_plan.py.  Built with plain g++ and no ROCm include path, like runnerup_plan_harness.cc.
#include "mgm_planner.h"

using namespace mgm;

extern "C" {

int consensus_request_bytes() { return (int)sizeof(ConsensusRequest); }
int consensus_choice_bytes() { return (int)sizeof(ConsensusChoice); }
long long consensus_wg_per_cu() { return kConsensusWgPerCu; }
long long consensus_rel_wg_per_cu() { return kConsensusRelWgPerCu; }

// `n` requests as their bytes, one after the other (integers only, no padding: static_assert in the header); per request
// out[7] = family, LPL, PPW, MAXD, SPL, per_wave, grid
void consensus_plan(const unsigned char *reqs, int n, long long *out)
{
    for (int i = 0; i < n; i++) {
        ConsensusRequest q;
        memcpy(&q, reqs + (size_t)i * sizeof q, sizeof q);
        const ConsensusChoice c = plan_wta_consensus(q);
        const long long v[7] = {c.family, c.LPL, c.PPW, c.MAXD, c.SPL, c.per_wave, c.grid};
        memcpy(out + (size_t)i * 7, v, sizeof v);
    }
}

}  // extern "C"
