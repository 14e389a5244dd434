/* Plain-C consumer of bsk_policy_* (include/bskgpu.h): a batch is reset from the ICs in argv[1], a policy (relu [16] action network,
 * relu [16] value network) is created from the float32 parameter block in argv[3], and bsk_policy_rollout closes the loop on the
 * device for six env steps of five sub-steps - no torch, no device allocator, no host visit in between.  A checksum of the
 * observations, a few numbers of the handle and the draw counter after a sampled rollout are printed; the test compares them with
 * the same calls through the Python binding. */
#include <stdio.h>
#include <stdlib.h>

#include "bskgpu.h"

#define CHECK(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, bsk_last_error()); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc < 4) return 9;
    const int n = atoi(argv[2]), n_rw = 4;
    bsk_config cfg;
    CHECK(bsk_default_config(&cfg, n_rw, BSK_GRAV_PM_J2));
    bsk_handle* h = NULL;
    CHECK(bsk_create(&cfg, n, 0, NULL, &h));
    const int nf = bsk_n_fields(h);
    double* ic = (double*)calloc((size_t)nf * n, sizeof(double));
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(ic, sizeof(double), (size_t)nf * n, f) != (size_t)nf * n) { fprintf(stderr, "cannot read ICs\n"); return 4; }
    fclose(f);
    CHECK(bsk_reset(h, NULL, ic));

    bsk_policy_spec spec = {0};
    spec.abi_version = BSK_ABI_VERSION;
    spec.struct_size = (uint32_t)sizeof spec;
    spec.n_hidden = 1; spec.hidden[0] = 16; spec.activation = BSK_POLICY_RELU;
    spec.has_value = 1; spec.v_n_hidden = 1; spec.v_hidden[0] = 16; spec.v_activation = BSK_POLICY_RELU;
    const int np = bsk_policy_n_params(&spec);
    if (np != 10 + (5 * 16 + 16) + (16 * 3 + 3) + (5 * 16 + 16) + (16 + 1)) return 5;
    float* params = (float*)malloc(sizeof(float) * (size_t)np);
    f = fopen(argv[3], "rb");
    if (!f || fread(params, sizeof(float), (size_t)np, f) != (size_t)np) { fprintf(stderr, "cannot read parameters\n"); return 4; }
    fclose(f);
    bsk_policy* p = NULL;
    CHECK(bsk_policy_create(&spec, params, 0, &p));
    int32_t* zero = (int32_t*)calloc((size_t)n, sizeof(int32_t));
    CHECK(bsk_step(h, zero, 5));                     /* the observation buffers hold a step's output */
    CHECK(bsk_policy_rollout(p, h, BSK_POLICY_GREEDY, 5, 6, NULL, NULL, NULL, NULL, NULL, NULL));
    double* obs = (double*)malloc(sizeof(double) * 5 * (size_t)n);
    double* rew = (double*)malloc(sizeof(double) * (size_t)n);
    double* st = (double*)malloc(sizeof(double) * (size_t)nf * n);
    uint8_t* why = (uint8_t*)malloc((size_t)n);
    CHECK(bsk_get_obs_state(h, obs, rew, why, st));
    double sum = 0.0;
    for (int j = 0; j < 5 * n; ++j) sum += obs[j];
    double rsum = 0; int64_t ndone = 0;
    CHECK(bsk_get_batch_stats(h, &rsum, &ndone));
    printf("%.17g %.17g %.17g %.17g %.17g ", sum, obs[0], rew[n - 1], st[(size_t)9 * n + 1], rsum);
    CHECK(bsk_policy_set_rng(p, 123456789012345ull, 40));
    CHECK(bsk_policy_rollout(p, h, BSK_POLICY_SAMPLE, 5, 3, NULL, NULL, NULL, NULL, NULL, NULL));
    uint64_t seed = 0, draw = 0;
    CHECK(bsk_policy_get_rng(p, &seed, &draw));
    CHECK(bsk_get_obs_state(h, obs, rew, why, st));
    sum = 0.0;
    for (int j = 0; j < 5 * n; ++j) sum += obs[j];
    printf("%llu %llu %.17g\n", (unsigned long long)seed, (unsigned long long)draw, sum);
    /* refusals */
    if (bsk_policy_rollout(p, h, 7, 5, 1, NULL, NULL, NULL, NULL, NULL, NULL) != BSK_EINVAL) return 6;
    if (bsk_policy_rollout(NULL, h, 0, 5, 1, NULL, NULL, NULL, NULL, NULL, NULL) != BSK_EINVAL) return 6;
    spec.hidden[0] = 20;
    if (bsk_policy_n_params(&spec) != BSK_EINVAL) return 7;
    bsk_policy_destroy(p);
    bsk_destroy(h);
    free(ic); free(params); free(zero); free(obs); free(rew); free(st); free(why);
    return 0;
}
