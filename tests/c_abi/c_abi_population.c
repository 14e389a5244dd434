/* Plain-C consumer of bsk_population_* (include/bskgpu.h): argv[4] members (relu [16] action networks, argv[3]: their float32
 * parameter blocks) drive argv[2] spacecraft reset from the ICs in argv[1], argv[2] / argv[4] each, through one generation -
 * bsk_population_rollout, six env steps of five sub-steps, gamma 0.97 - and the per-member fitness and mean episode length formed on
 * the device are printed; then the members are handed over again from DEVICE memory, rotated by one, and the fitness printed once
 * more.  The test compares the printout with the same calls through the Python binding.  The three HIP runtime calls a C program
 * needs to own device memory are declared here: the library's header is the only one included. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bskgpu.h"

int hipMalloc(void** ptr, size_t size);
int hipMemcpy(void* dst, const void* src, size_t size, int kind);      /* kind 1: host to device, 2: device to host */
int hipFree(void* ptr);

#define CHECK(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, bsk_last_error()); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc < 5) return 9;
    const int n = atoi(argv[2]), P = atoi(argv[4]), n_rw = 4;
    bsk_config cfg;
    CHECK(bsk_default_config(&cfg, n_rw, BSK_GRAV_PM_J2));
    bsk_handle* h = NULL;
    CHECK(bsk_create(&cfg, n, 0, NULL, &h));
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
    const size_t total = (size_t)np * (size_t)P;
    float* params = (float*)malloc(sizeof(float) * total);
    f = fopen(argv[3], "rb");
    if (!f || fread(params, sizeof(float), total, f) != total) { fprintf(stderr, "cannot read parameters\n"); return 4; }
    fclose(f);
    bsk_population* pop = NULL;
    CHECK(bsk_population_create(&spec, P, params, 0, &pop));

    int32_t* zero = (int32_t*)calloc((size_t)n, sizeof(int32_t));
    double* d_out = NULL;                             /* fitness[P], then mean_len[P] */
    float* d_params = NULL;
    if (hipMalloc((void**)&d_out, sizeof(double) * 2 * (size_t)P) || hipMalloc((void**)&d_params, sizeof(float) * total)) return 3;
    double* out = (double*)malloc(sizeof(double) * 2 * (size_t)P);
    for (int round = 0; round < 2; ++round) {
        CHECK(bsk_reset(h, NULL, ic));
        CHECK(bsk_step(h, zero, 5));                  /* the observation buffers hold a step's output */
        CHECK(bsk_population_rollout(pop, h, BSK_POLICY_GREEDY, 5, 6, 0.97, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, d_out, d_out + P));
        CHECK(bsk_sync(h));
        if (hipMemcpy(out, d_out, sizeof(double) * 2 * (size_t)P, 2)) return 3;
        for (int m = 0; m < 2 * P; ++m) printf("%.17g ", out[m]);
        if (round == 0) {
            /* the members again, rotated by one, from device memory: member m takes block m + 1, the last one block 0 */
            if (hipMemcpy(d_params, params + np, sizeof(float) * (total - (size_t)np), 1)) return 3;
            if (hipMemcpy(d_params + (total - (size_t)np), params, sizeof(float) * (size_t)np, 1)) return 3;
            CHECK(bsk_population_set_params_device(pop, d_params, 0, P, NULL));
            float* back = (float*)malloc(sizeof(float) * (size_t)np);
            CHECK(bsk_population_get_member(pop, P - 1, back));
            if (memcmp(back, params, sizeof(float) * (size_t)np) != 0) return 8;
            free(back);
        }
    }
    printf("\n");
    /* refusals */
    if (bsk_population_rollout(pop, h, 7, 5, 1, 1.0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) != BSK_EINVAL) return 6;
    if (bsk_population_rollout(NULL, h, 0, 5, 1, 1.0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) != BSK_EINVAL) return 6;
    if (bsk_population_set_params_device(pop, d_params, 1, P, NULL) != BSK_EINVAL) return 6;
    bsk_population* none = NULL;
    if (bsk_population_create(&spec, 0, params, 0, &none) != BSK_EINVAL || none) return 7;
    bsk_population_destroy(pop);
    bsk_destroy(h);
    if (hipFree(d_out) || hipFree(d_params)) return 3;
    free(ic); free(params); free(zero); free(out);
    return 0;
}
