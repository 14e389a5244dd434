// bsk_envstep.hpp — how an episode starts on the device, one definition each (internal).
//   pool_slot          the IC-pool slot an episode restarts from: step_kernel's auto-reset, rollout_kernel's restart,
//                      reset_from_pool_kernel, reset_from_pool_shared_kernel
//   first_observation  what a reset leaves in the observation buffers: step_kernel's auto-reset, rollout_kernel's restart,
//                      init_outputs (bsk_aux.hip)
// The floating-point operations are in one fixed order (explicit sqrt_nr), so every caller gets the same bits.
// (oracle/bsk_oracle.c restates both independently, on purpose.)
#pragma once
#include "bsk_device.hpp"

namespace bsk {

// ---- IC pool: slot of (env | shared member env, finished episodes | epoch), include/bskgpu.h: bsk_set_ic_pool, bsk_reset_from_pool_shared
__device__ __forceinline__ unsigned pool_slot(unsigned key, unsigned episode_or_epoch, unsigned n_pool) {
    return (key * 2654435761u + episode_or_epoch * 40503u + 12345u) % n_pool;
}

// ---- the new episode's first observation (the vec env's convention): |sigma_BN|, |omega|, |Omega| / limit, charge / 3600 / power_max, 1
struct Obs5 { double o[5]; };
__device__ __forceinline__ Obs5 first_observation(V3 sigma, V3 omega, double om2, double charge, double inv_wheel_limit, double charge_scale) {
    return Obs5{{sqrt_nr(dot(sigma, sigma)), sqrt_nr(dot(omega, omega)), sqrt_nr(om2) * inv_wheel_limit, charge * charge_scale, 1.0}};
}

}  // namespace bsk
