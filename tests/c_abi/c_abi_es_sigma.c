/* Plain-C consumer of the evolution strategy's per-parameter step size (include/bskgpu.h, bsk_es_set_sigma_adaptation): a relu [16]
 * action network (argv[3]: the float32 parameter block it starts from) searched with argv[4] members over 128 spacecraft that
 * restart from the pool of argv[2] initial conditions in argv[1].  BSK_ES_SIGMA_PGPE is selected (lr_sigma 0.5, at most 0.2 of
 * itself per generation, inside [0.01, 1]) and bsk_es_set_sigma gives parameter j the step size 0.05 + 0.001 * (j mod 100); two
 * generations under SGD - bsk_reset_from_pool_shared under the optimiser's generation word, bsk_es_ask, bsk_population_rollout (six
 * env steps of five sub-steps, gamma 0.97) with the fitness left in device memory, bsk_es_tell - all on the handle's stream.  The
 * fitness of each generation, then theta, sigma_vec and the generation counter are printed as hex floats; the test compares the
 * printout with the same calls through the Python binding.  The three HIP runtime calls a C program needs to own device memory
 * are declared here: the library's header is the only one included. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bskgpu.h"

int hipMalloc(void** ptr, size_t size);
int hipMemcpy(void* dst, const void* src, size_t size, int kind);      /* kind 2: device to host */
int hipFree(void* ptr);

#define CHECK(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, bsk_last_error()); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc < 5) return 9;
    const int n = 128, n_pool = atoi(argv[2]), P = atoi(argv[4]), n_rw = 4;
    if (n_pool < 1 || P < 2 || n % P) return 9;
    const int E = n / P;
    bsk_config cfg;
    CHECK(bsk_default_config(&cfg, n_rw, BSK_GRAV_PM_J2));
    cfg.flags |= BSK_FLAG_AUTO_RESET;
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
    bsk_population* pop = NULL;
    CHECK(bsk_population_create(&spec, P, NULL, 0, &pop));
    bsk_es* es = NULL;
    const uint64_t seed = ((uint64_t)1 << 33) + 5;
    CHECK(bsk_es_create(&spec, P, theta0, 0.1, 0.05, 10, seed, 0, &es));
    double* sigma = (double*)malloc(sizeof(double) * (size_t)np);
    /* refusals: no vector while the kind is FIXED, arguments outside their ranges, an unknown kind, a bad entry */
    if (bsk_es_get_sigma(es, sigma) != BSK_EINVAL || bsk_es_set_sigma(es, sigma) != BSK_EINVAL) return 7;
    if (bsk_es_set_sigma_adaptation(es, 2, 0.5, 0.2, 0.01, 1.0) != BSK_EINVAL) return 7;
    if (bsk_es_set_sigma_adaptation(es, BSK_ES_SIGMA_PGPE, -0.5, 0.2, 0.01, 1.0) != BSK_EINVAL) return 7;
    if (bsk_es_set_sigma_adaptation(es, BSK_ES_SIGMA_PGPE, 0.5, 1.0, 0.01, 1.0) != BSK_EINVAL) return 7;
    if (bsk_es_set_sigma_adaptation(es, BSK_ES_SIGMA_PGPE, 0.5, 0.2, 0.0, 1.0) != BSK_EINVAL) return 7;
    if (bsk_es_set_sigma_adaptation(es, BSK_ES_SIGMA_PGPE, 0.5, 0.2, 0.2, 1.0) != BSK_EINVAL) return 7;      /* sigma = 0.1 below sigma_min */
    if (bsk_es_get_sigma(es, sigma) != BSK_EINVAL) return 7;
    CHECK(bsk_es_set_sigma_adaptation(es, BSK_ES_SIGMA_PGPE, 0.5, 0.2, 0.01, 1.0));
    CHECK(bsk_es_get_sigma(es, sigma));
    for (int j = 0; j < np; ++j)
        if (sigma[j] != 0.1) return 8;
    sigma[3] = 0.0;
    if (bsk_es_set_sigma(es, sigma) != BSK_EINVAL) return 7;
    for (int j = 0; j < np; ++j) sigma[j] = 0.05 + 0.001 * (double)(j % 100);
    CHECK(bsk_es_set_sigma(es, sigma));
    const uint64_t* d_generation = NULL;
    CHECK(bsk_es_generation_device(es, &d_generation));
    if (!d_generation) return 8;

    double* d_fitness = NULL;
    if (hipMalloc((void**)&d_fitness, sizeof(double) * (size_t)P)) return 3;
    double* fitness = (double*)malloc(sizeof(double) * (size_t)P);
    for (int g = 0; g < 2; ++g) {
        CHECK(bsk_reset_from_pool_shared(h, E, d_generation, NULL));
        CHECK(bsk_es_ask(es, pop, stream));
        CHECK(bsk_population_rollout(pop, h, BSK_POLICY_GREEDY, 5, 6, 0.97, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, d_fitness, NULL));
        CHECK(bsk_es_tell(es, d_fitness, stream));
        CHECK(bsk_sync(h));
        if (hipMemcpy(fitness, d_fitness, sizeof(double) * (size_t)P, 2)) return 3;
        for (int k = 0; k < P; ++k) printf("%a ", fitness[k]);
    }
    double* theta = (double*)malloc(sizeof(double) * (size_t)np);
    uint64_t generation = 99;
    CHECK(bsk_es_get_state(es, theta, &generation));
    CHECK(bsk_es_get_sigma(es, sigma));
    for (int j = 0; j < np; ++j) printf("%a ", theta[j]);
    for (int j = 0; j < np; ++j) printf("%a ", sigma[j]);
    printf("%a\n", (double)generation);
    for (int j = 0; j < 10; ++j)
        if (theta[j] != (double)theta0[j] || sigma[j] != 0.05 + 0.001 * (double)j) return 8;     /* frozen: carried, never moved */
    /* FIXED gives the vector up again, and selecting PGPE again fills it with the creation sigma */
    CHECK(bsk_es_set_sigma_adaptation(es, BSK_ES_SIGMA_FIXED, -1.0, 7.0, 0.0, -1.0));
    if (bsk_es_get_sigma(es, sigma) != BSK_EINVAL) return 7;
    CHECK(bsk_es_set_sigma_adaptation(es, BSK_ES_SIGMA_PGPE, 0.0, 0.5, 0.1, 0.1));
    CHECK(bsk_es_get_sigma(es, sigma));
    for (int j = 0; j < np; ++j)
        if (sigma[j] != 0.1) return 8;
    bsk_es_destroy(es);
    bsk_population_destroy(pop);
    bsk_destroy(h);
    if (hipFree(d_fitness)) return 3;
    free(pool); free(theta0); free(fitness); free(theta); free(sigma);
    return 0;
}
