/* Plain-C consumer of the evolution strategy's validation on fixed episodes (include/bskgpu.h, bsk_es_set_validation): a relu [16]
 * action network (argv[3]: the float32 parameter block it starts from) searched with argv[4] members and validated with argv[5]
 * more that hold the centre, 64 spacecraft each, restarting from the pool of argv[2] initial conditions in argv[1].  Two generations
 * under SGD, all on the handle's stream: the training envs restart by bsk_reset_from_pool_shared under the optimiser's generation
 * word and a device mask of their own, validation member v's under the epoch word v of bsk_es_validation_epochs_device and its
 * mask; bsk_es_ask into the argv[4] + argv[5] members; bsk_population_rollout (six env steps of two sub-steps, gamma 0.97) with
 * fitness and mean lengths left in device memory; bsk_es_tell.  The two validation rows, the validated champion and theta are
 * printed as hex floats; the test compares the printout with the same loop through the Python binding.  The three HIP runtime
 * calls a C program needs to own device memory are declared here: the library's header is the only one included. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bskgpu.h"

int hipMalloc(void** ptr, size_t size);
int hipMemcpy(void* dst, const void* src, size_t size, int kind);      /* kind 1: host to device, 2: device to host */
int hipFree(void* ptr);

#define CHECK(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, bsk_last_error()); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc < 6) return 9;
    const int n_pool = atoi(argv[2]), P = atoi(argv[4]), V = atoi(argv[5]), E = 64, n_rw = 4, C = 4;
    if (n_pool < 1 || P < 2 || V < 1 || V > 16) return 9;
    const int n = (P + V) * E;
    bsk_config cfg;
    CHECK(bsk_default_config(&cfg, n_rw, BSK_GRAV_PM_J2));
    cfg.flags |= BSK_FLAG_AUTO_RESET;
    cfg.max_length = 4;
    bsk_handle* h = NULL;
    CHECK(bsk_create(&cfg, n, 0, NULL, &h));
    void* stream = NULL;
    CHECK(bsk_get_stream(h, &stream));
    const int nf = bsk_n_fields(h);
    double* pool = (double*)calloc((size_t)nf * n_pool, sizeof(double));
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(pool, sizeof(double), (size_t)nf * n_pool, f) != (size_t)nf * n_pool) { fprintf(stderr, "cannot read the pool\n"); return 4; }
    fclose(f);
    CHECK(bsk_set_ic_pool(h, n_pool, pool));

    bsk_policy_spec spec;
    memset(&spec, 0, sizeof spec);
    spec.abi_version = BSK_ABI_VERSION;
    spec.struct_size = (uint32_t)sizeof spec;
    spec.n_hidden = 1; spec.hidden[0] = 16; spec.activation = BSK_POLICY_RELU;
    const int np = bsk_policy_n_params(&spec);
    if (np != 10 + (5 * 16 + 16) + (16 * 3 + 3)) return 5;
    float* theta0 = (float*)malloc(sizeof(float) * (size_t)np);
    f = fopen(argv[3], "rb");
    if (!f || fread(theta0, sizeof(float), (size_t)np, f) != (size_t)np) { fprintf(stderr, "cannot read parameters\n"); return 4; }
    fclose(f);
    bsk_population *pop = NULL, *small = NULL;
    CHECK(bsk_population_create(&spec, P + V, NULL, 0, &pop));
    CHECK(bsk_population_create(&spec, P, NULL, 0, &small));
    bsk_es* es = NULL;
    const uint64_t seed = ((uint64_t)1 << 33) + 5, epoch0 = 0xFFFFFFFFull;
    CHECK(bsk_es_create(&spec, P, theta0, 0.1, 0.05, 10, seed, 0, &es));

    double *d_fitness = NULL, *d_len = NULL;
    uint8_t* d_mask = NULL;
    if (hipMalloc((void**)&d_fitness, sizeof(double) * (size_t)(P + V)) || hipMalloc((void**)&d_len, sizeof(double) * (size_t)(P + V)) ||
        hipMalloc((void**)&d_mask, (size_t)(1 + V) * (size_t)n))
        return 3;
    /* row 0: the envs of the P training members; row 1 + v: those of validation member v */
    uint8_t* mask = (uint8_t*)calloc((size_t)(1 + V) * (size_t)n, 1);
    memset(mask, 1, (size_t)P * E);
    for (int v = 0; v < V; ++v) memset(mask + (size_t)(1 + v) * n + (size_t)(P + v) * E, 1, (size_t)E);
    if (hipMemcpy(d_mask, mask, (size_t)(1 + V) * (size_t)n, 1)) return 3;

    /* refusals: with validation off nothing of it exists and the larger population is the wrong one; arguments outside their ranges */
    const uint64_t* d_epochs = NULL;
    const float* d_best = NULL;
    uint64_t gen[4];
    double rows[16];
    if (bsk_es_validation_epochs_device(es, &d_epochs) != BSK_EINVAL || bsk_es_validated_best_device(es, &d_best) != BSK_EINVAL) return 7;
    if (bsk_es_get_validation_log(es, gen, rows) != BSK_EINVAL || bsk_es_get_validated_best(es, NULL, NULL, NULL) != BSK_EINVAL) return 7;
    if (bsk_es_ask(es, pop, stream) != BSK_EINVAL) return 7;
    if (bsk_es_set_validation(NULL, V, C, epoch0, d_len) != BSK_EINVAL || bsk_es_set_validation(es, 17, C, epoch0, d_len) != BSK_EINVAL) return 7;
    if (bsk_es_set_validation(es, -1, C, epoch0, d_len) != BSK_EINVAL || bsk_es_set_validation(es, V, 0, epoch0, d_len) != BSK_EINVAL) return 7;
    if (bsk_population_set_obs_stats_members(pop, 0) != BSK_EINVAL || bsk_population_set_obs_stats_members(pop, P + V + 1) != BSK_EINVAL) return 7;
    if (bsk_es_validation_epochs_device(es, &d_epochs) != BSK_EINVAL) return 7;
    CHECK(bsk_es_set_validation(es, V, C, epoch0, d_len));
    if (bsk_es_ask(es, small, stream) != BSK_EINVAL) return 7;               /* now the population of P members is the wrong one */
    CHECK(bsk_es_validation_epochs_device(es, &d_epochs));
    CHECK(bsk_es_validated_best_device(es, &d_best));
    if (!d_epochs || !d_best) return 8;
    uint64_t epochs[16];
    if (hipMemcpy(epochs, d_epochs, sizeof(uint64_t) * (size_t)V, 2)) return 3;
    for (int v = 0; v < V; ++v)
        if (epochs[v] != epoch0 + (uint64_t)v) return 8;
    CHECK(bsk_es_get_validation_log(es, gen, rows));
    for (int c = 0; c < C; ++c)
        if (gen[c] != ~(uint64_t)0 || rows[4 * c] != 0.0) return 8;
    const uint64_t* d_generation = NULL;
    CHECK(bsk_es_generation_device(es, &d_generation));

    for (int g = 0; g < 2; ++g) {
        CHECK(bsk_reset_from_pool_shared(h, E, d_generation, d_mask));
        for (int v = 0; v < V; ++v) CHECK(bsk_reset_from_pool_shared(h, E, d_epochs + v, d_mask + (size_t)(1 + v) * n));
        CHECK(bsk_es_ask(es, pop, stream));
        CHECK(bsk_population_rollout(pop, h, BSK_POLICY_GREEDY, 2, 6, 0.97, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, d_fitness, d_len));
        CHECK(bsk_es_tell(es, d_fitness, stream));
    }
    CHECK(bsk_sync(h));
    CHECK(bsk_es_get_validation_log(es, gen, rows));
    for (int g = 0; g < 2; ++g) {
        if (gen[g] != (uint64_t)g || rows[4 * g + 3] != (double)V) return 8;
        for (int c = 0; c < 4; ++c) printf("%a ", rows[4 * g + c]);
    }
    if (gen[2] != ~(uint64_t)0 || gen[3] != ~(uint64_t)0) return 8;
    float* best = (float*)malloc(sizeof(float) * (size_t)np);
    float* best_dev = (float*)malloc(sizeof(float) * (size_t)np);
    double best_fitness = 0.0;
    uint64_t best_generation = 99, generation = 99;
    CHECK(bsk_es_get_validated_best(es, best, &best_fitness, &best_generation));
    if (hipMemcpy(best_dev, d_best, sizeof(float) * (size_t)np, 2)) return 3;
    if (memcmp(best, best_dev, sizeof(float) * (size_t)np) != 0) return 8;
    printf("%a %a ", best_fitness, (double)best_generation);
    for (int j = 0; j < np; ++j) printf("%a ", (double)best[j]);
    double* theta = (double*)malloc(sizeof(double) * (size_t)np);
    CHECK(bsk_es_get_state(es, theta, &generation));
    for (int j = 0; j < np; ++j) printf("%a ", theta[j]);
    printf("%a\n", (double)generation);
    /* the champion round trip, and off again: nothing of it exists, and the population of P members is the right one */
    const double one = 1.0;
    CHECK(bsk_es_set_validated_best(es, NULL, &one, NULL));
    CHECK(bsk_es_get_validated_best(es, NULL, &best_fitness, NULL));
    if (best_fitness != 1.0) return 8;
    CHECK(bsk_es_set_validation(es, 0, 0, 0, NULL));
    if (bsk_es_get_validation_log(es, gen, rows) != BSK_EINVAL || bsk_es_ask(es, pop, stream) != BSK_EINVAL) return 7;
    CHECK(bsk_es_ask(es, small, stream));
    CHECK(bsk_sync(h));
    bsk_es_destroy(es);
    bsk_population_destroy(pop);
    bsk_population_destroy(small);
    bsk_destroy(h);
    if (hipFree(d_fitness) || hipFree(d_len) || hipFree(d_mask)) return 3;
    free(pool); free(theta0); free(mask); free(best); free(best_dev); free(theta);
    return 0;
}
