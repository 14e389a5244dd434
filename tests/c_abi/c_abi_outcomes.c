/* Plain-C consumer of bsk_population_set_outcomes (include/bskgpu.h): argv[4] members (relu [16] action networks, argv[3]: their
 * float32 parameter blocks) drive argv[2] spacecraft reset from the ICs in argv[1], argv[2] / argv[4] each, through one generation -
 * bsk_population_rollout, six env steps of five sub-steps, gamma 0.97, episodes of at most four steps - with episode-outcome rows
 * attached, and the rows formed on the device are printed, BSK_OUTCOME_COLS numbers per member.  The test compares the printout
 * with the same calls through the Python binding.  The three HIP runtime calls a C program needs to own device memory are
 * declared here: the library's header is the only one included. */
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
    cfg.max_length = 4;
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
    const size_t words = (size_t)BSK_OUTCOME_COLS * (size_t)P;
    double* d_rows = NULL;
    if (hipMalloc((void**)&d_rows, sizeof(double) * words)) return 3;
    double* rows = (double*)malloc(sizeof(double) * words);
    CHECK(bsk_reset(h, NULL, ic));
    CHECK(bsk_step(h, zero, 5));                      /* the observation buffers hold a step's output */
    CHECK(bsk_population_set_outcomes(pop, d_rows));
    /* no fitness output, no history: the rows alone */
    CHECK(bsk_population_rollout(pop, h, BSK_POLICY_GREEDY, 5, 6, 0.97, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL));
    CHECK(bsk_sync(h));
    if (hipMemcpy(rows, d_rows, sizeof(double) * words, 2)) return 3;
    for (size_t k = 0; k < words; ++k) printf("%.17g ", rows[k]);
    printf("\n");
    /* detached again: the rollout runs as it always has; and the one refusal of the attach */
    CHECK(bsk_population_set_outcomes(pop, NULL));
    CHECK(bsk_population_rollout(pop, h, BSK_POLICY_GREEDY, 5, 1, 0.97, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL));
    CHECK(bsk_sync(h));
    if (bsk_population_set_outcomes(NULL, d_rows) != BSK_EINVAL) return 6;
    bsk_population_destroy(pop);
    bsk_destroy(h);
    if (hipFree(d_rows)) return 3;
    free(ic); free(params); free(zero); free(rows);
    return 0;
}
