/* Plain-C consumer of bsk_es_* (include/bskgpu.h): an evolution strategy over a relu [16] action network (argv[3]: the float32
 * parameter block it starts from) with argv[4] members, each driving argv[2] / argv[4] of the argv[2] spacecraft reset from the ICs
 * in argv[1].  Two generations - bsk_es_ask, bsk_population_rollout (six env steps of five sub-steps, gamma 0.97) with the fitness
 * left in device memory, bsk_es_tell - all on the handle's stream; the fitness of each generation, then theta and the generation
 * counter are printed.  The test compares the printout with the same calls through the Python binding.  The three HIP runtime
 * calls a C program needs to own device memory are declared here: the library's header is the only one included. */
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
    const int n = atoi(argv[2]), P = atoi(argv[4]), n_rw = 4;
    bsk_config cfg;
    CHECK(bsk_default_config(&cfg, n_rw, BSK_GRAV_PM_J2));
    bsk_handle* h = NULL;
    CHECK(bsk_create(&cfg, n, 0, NULL, &h));
    void* stream = NULL;
    CHECK(bsk_get_stream(h, &stream));
    const int nf = bsk_n_fields(h);
    double* ic = (double*)calloc((size_t)nf * n, sizeof(double));
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(ic, sizeof(double), (size_t)nf * n, f) != (size_t)nf * n) { fprintf(stderr, "cannot read ICs\n"); return 4; }
    fclose(f);

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

    int32_t* zero = (int32_t*)calloc((size_t)n, sizeof(int32_t));
    double* d_fitness = NULL;
    if (hipMalloc((void**)&d_fitness, sizeof(double) * (size_t)P)) return 3;
    double* fitness = (double*)malloc(sizeof(double) * (size_t)P);
    for (int g = 0; g < 2; ++g) {
        CHECK(bsk_reset(h, NULL, ic));
        CHECK(bsk_step(h, zero, 5));                  /* the observation buffers hold a step's output */
        CHECK(bsk_es_ask(es, pop, stream));
        CHECK(bsk_population_rollout(pop, h, BSK_POLICY_GREEDY, 5, 6, 0.97, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, d_fitness, NULL));
        CHECK(bsk_es_tell(es, d_fitness, stream));
        CHECK(bsk_sync(h));
        if (hipMemcpy(fitness, d_fitness, sizeof(double) * (size_t)P, 2)) return 3;
        for (int m = 0; m < P; ++m) printf("%.17g ", fitness[m]);
    }
    double* theta = (double*)malloc(sizeof(double) * (size_t)np);
    uint64_t generation = 99;
    CHECK(bsk_es_get_state(es, theta, &generation));
    for (int j = 0; j < np; ++j) printf("%.17g ", theta[j]);
    printf("%d\n", (int)generation);
    for (int j = 0; j < 10; ++j)
        if (theta[j] != (double)theta0[j]) return 8;       /* in_scale / in_shift never move */
    /* refusals */
    bsk_es* none = NULL;
    if (bsk_es_create(&spec, P + 1, theta0, 0.1, 0.05, 10, seed, 0, &none) != BSK_EINVAL || none) return 7;
    if (bsk_es_create(&spec, P, theta0, 0.0, 0.05, 10, seed, 0, &none) != BSK_EINVAL || none) return 7;
    if (bsk_es_ask(es, NULL, stream) != BSK_EINVAL || bsk_es_tell(es, NULL, stream) != BSK_EINVAL) return 6;
    CHECK(bsk_es_set_state(es, NULL, 7));
    CHECK(bsk_es_get_state(es, NULL, &generation));
    if (generation != 7) return 8;
    bsk_es_destroy(es);
    bsk_population_destroy(pop);
    bsk_destroy(h);
    if (hipFree(d_fitness)) return 3;
    free(ic); free(theta0); free(zero); free(fitness); free(theta);
    return 0;
}
