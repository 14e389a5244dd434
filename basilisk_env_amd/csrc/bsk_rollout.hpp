// bsk_rollout.hpp — host-side entry points of the open-loop rollout kernel (bsk_rollout.hip; internal).
#pragma once
#include "bsk_launch.hpp"

namespace bsk {

struct RolloutBuffers {
    const int* actions;            // [T][n] device, or NULL: `const_action` at every step
    double* obs_hist;              // [T][5][n] device (NULL: not recorded)
    double* reward_hist;           // [T][n]
    unsigned char* reason_hist;    // [T][n]
    int n_steps, const_action;
};

struct RolloutLaunch : StepLaunch { const RolloutBuffers& r; };

// built for: point mass / J2 at the bare level (every wheel set, diagonal and general hub)
bool rollout_available(int grav, int feat);
// the rollout kernel of (gravity model, wheels, hub kind, per-step actions or not), as dispatch_step (bsk_launch.hpp) does it
hipError_t dispatch_rollout(int grav, int nrw, bool diag, bool act, int block, int n, const RolloutLaunch* go, KernelDesc* d);

}  // namespace bsk
