// bsk_capi_policy.hpp — what bsk_capi_policy.hip (policy, population, observation statistics) and bsk_capi_es.hip (evolution
// strategy) share: the objects an optimiser reads through their handles, the create / destroy skeleton of everything made from a
// bsk_policy_spec, and the transfer behind every get / set pair.  Internal, by bsk_capi.hpp's rule: not installed, nothing here is
// exported - everything that crosses a translation unit lives in bsk::capi, a namespace of hidden visibility.
#pragma once
#include <initializer_list>

#include "bsk_capi.hpp"
#include "bsk_obsstats.hpp"
#include "bsk_policy.hpp"
#include "bsk_population.hpp"

// bsk_obs_stats_*: sums, sums of squares and counts of the observation rows (kernels: bsk_obsstats.hip)
struct bsk_obs_stats {
    int device = 0;
    int n_cap = 0;
    void* d_block = nullptr;               // ONE allocation of 8-byte words: [part | cnt | tot | tot_n]
    bsk::ObsStats st = {};
    size_t words() const { return (size_t)st.waves * 11 + 11; }
};

namespace bsk { namespace capi __attribute__((visibility("hidden"))) {

// What a policy and a population are alike in: n_members parameter blocks of one spec on one device (a policy: one block) and
// one draw counter for all of them
struct ParamStore {
    bsk::PolicyLayout lay;
    int device = 0;
    int n_members = 1;
    float* d_params = nullptr;             // [n_members][lay.n_device]: one device layout of the parameters (bsk_policy.hpp) per member
    unsigned long long* d_rng = nullptr;   // {seed, draw}: read by sample-mode launches, draw advanced behind each of them
    bsk_obs_stats* stats = nullptr;        // bsk_*_set_obs_stats: what the rollouts accumulate into; not owned
    int n_counted = 0;                     // bsk_population_set_obs_stats_members: the envs of the first n_counted members feed `stats`; 0: all
};

// (one definition of each: bsk_capi_policy.hip)
int policy_spec_layout(const bsk_policy_spec* spec, bsk::PolicyLayout& lay);
// The destroy rule: what is queued on the device may still use the buffers - wait for it once if there is any, then free them
void free_all(std::initializer_list<void*> bufs);

// The create skeleton of the three objects.  Its head: *out = NULL, then the spec's layout ...
template <class T>
int create_begin(const bsk_policy_spec* spec, T** out, bsk::PolicyLayout& lay) {
    if (!out) return fail(BSK_EINVAL, "out is NULL");
    *out = nullptr;
    return policy_spec_layout(spec, lay);
}

// ... and, behind the caller's own argument checks, its tail: admit the device, allocate through `init`, destroy what a failure leaves
template <class T, class Init>
int create_on_device(const bsk::PolicyLayout& lay, int device_id, T** out, void (*destroy)(T*), Init init) {
    int rc = open_device(device_id);
    if (rc) return rc;
    DeviceGuard guard(device_id);
    T* obj = new T();
    obj->lay = lay;
    obj->device = device_id;
    if ((rc = init(obj))) { destroy(obj); return rc; }
    *out = obj;
    return BSK_OK;
}

// What every get / set pair is behind its own refusals.  A field of the object: where the host has (or wants) it - NULL: the
// caller passes on it - where it lives on the device, and its size.
struct Field {
    const void* host;
    const void* dev;
    size_t bytes;
};
// dir = hipMemcpyDeviceToHost (a get) or hipMemcpyHostToDevice (a set): on `device`, ONE counted synchronisation - everything
// queued has written what a get reads, and has read what a set replaces - then one counted copy per field whose host is not NULL
int transfer(int device, hipMemcpyKind dir, std::initializer_list<Field> fields);

// A scratch buffer an enqueue-only entry point owns is replaced by one of `bytes`: refused with BSK_EINVAL and `capture_msg` while
// `stream` is being captured; a queued launch may still use the smaller buffer, so the device is waited for before that is freed.
// The caller decides when, and records the new capacity.
int grow_scratch(void** d_buf, int* cap, size_t bytes, hipStream_t stream, const char* capture_msg);

} }  // namespace bsk::capi

// bsk_policy_*: the fused MLP policy (kernel and layout: bsk_policy.hip)
struct bsk_policy : bsk::capi::ParamStore {
    int* d_act = nullptr;                  // bsk_policy_rollout's scratch row of actions (d_action_hist == NULL)
    int act_cap = 0;
};

// bsk_population_*: n_members parameter blocks of one spec, member m driving envs [m * E, (m + 1) * E) (bsk_policy.hip,
// bsk_population.hip)
struct bsk_population : bsk::capi::ParamStore {
    // bsk_population_rollout's scratch, one allocation sized for the largest handle seen: the running value of every env and a
    // row of actions (d_action_hist == NULL)
    void* d_scratch = nullptr;
    bsk::FitnessAcc acc = {};
    int* d_act = nullptr;
    int scratch_cap = 0;
    // bsk_population_set_outcomes: the caller's rows (NULL: off), and the second accumulator set - its own allocation, made by the
    // first rollout of a size that has rows attached
    double* d_outcomes = nullptr;
    void* d_out_scratch = nullptr;
    bsk::OutcomeAcc out = {};
    int out_cap = 0;
};
