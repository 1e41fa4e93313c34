// energy_plan_harness.cc -- plan_energy_copy and plan_energy_launch (mgm_amd/csrc/mgm_energyplan.h) behind a C interface for
// tests/test_energy_model_ref.py.  Built with plain g++ and no ROCm include path, like the other plan harnesses.
#include <cstring>

#include "mgm_energyplan.h"

using namespace mgm;

extern "C" {

int energy_request_ints() { return (int)(sizeof(EnergyCopyRequest) / sizeof(int)); }
int energy_threads() { return kEnergyThreads; }

// `n` requests as their ints, one after the other; per request out[3] = copy, cb, stride
void energy_copy_plan(const int *reqs, int n, int *out)
{
    for (int i = 0; i < n; i++) {
        EnergyCopyRequest q;
        memcpy(&q, reqs + (size_t)i * (sizeof q / sizeof(int)), sizeof q);
        const EnergyCopyChoice c = plan_energy_copy(q);
        out[3 * i] = c.copy, out[3 * i + 1] = c.cb, out[3 * i + 2] = c.stride;
    }
}

// out[2] = blocks, partial_bytes
void energy_launch_plan(int nx, int ny, long long *out)
{
    const EnergyLaunch l = plan_energy_launch(nx, ny);
    out[0] = l.blocks, out[1] = l.partial_bytes;
}

}  // extern "C"
