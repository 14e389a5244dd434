/* Plain-C consumer of bsk_fit_* (include/bskgpu.h): a policy (relu [16] action network) is created from the float32 parameter block
 * in argv[1], a fit is attached, and one bsk_fit_accumulate over the n = argv[4] observations (f64[5][n]) of argv[2] with the int32
 * labels of argv[3] is followed by one bsk_fit_step - no torch, no device allocator but the runtime's.  The diagnostics row,
 * theta[10..13], the step counter and beta_pow are printed as hex floats; the test compares them with the same calls through the
 * Python binding. */
#include <stdio.h>
#include <stdlib.h>

#include "bskgpu.h"

int hipMalloc(void** ptr, size_t size);
int hipMemcpy(void* dst, const void* src, size_t size, int kind);      /* kind 1: host to device, 2: device to host */
int hipFree(void* ptr);

#define CHECK(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, bsk_last_error()); return 1; } } while (0)

static void* read_file(const char* path, size_t bytes) {
    void* buf = malloc(bytes);
    FILE* f = fopen(path, "rb");
    if (!buf || !f || fread(buf, 1, bytes, f) != bytes) { fprintf(stderr, "cannot read %s\n", path); exit(4); }
    fclose(f);
    return buf;
}

int main(int argc, char** argv) {
    if (argc < 5) return 9;
    const int n = atoi(argv[4]);
    bsk_policy_spec spec = {0};
    spec.abi_version = BSK_ABI_VERSION;
    spec.struct_size = (uint32_t)sizeof spec;
    spec.n_hidden = 1; spec.hidden[0] = 16; spec.activation = BSK_POLICY_RELU;
    const int np = bsk_policy_n_params(&spec);
    if (np != 10 + (5 * 16 + 16) + (16 * 3 + 3)) return 5;
    float* params = (float*)read_file(argv[1], sizeof(float) * (size_t)np);
    double* obs = (double*)read_file(argv[2], sizeof(double) * 5 * (size_t)n);
    int32_t* labels = (int32_t*)read_file(argv[3], sizeof(int32_t) * (size_t)n);
    bsk_policy* p = NULL;
    CHECK(bsk_policy_create(&spec, params, 0, &p));
    bsk_fit* fit = NULL;
    CHECK(bsk_fit_create(p, 1e-2, 0.9, 0.999, 1e-8, 1e-3, 0.5, &fit));

    double* d_obs = NULL;
    int32_t* d_labels = NULL;
    if (hipMalloc((void**)&d_obs, sizeof(double) * 5 * (size_t)n) || hipMalloc((void**)&d_labels, sizeof(int32_t) * (size_t)n)) return 3;
    if (hipMemcpy(d_obs, obs, sizeof(double) * 5 * (size_t)n, 1) || hipMemcpy(d_labels, labels, sizeof(int32_t) * (size_t)n, 1)) return 3;
    CHECK(bsk_fit_accumulate(fit, d_obs, n, n, d_labels, NULL, NULL, NULL, 0, NULL));
    CHECK(bsk_fit_step(fit, NULL));

    const double* d_row = NULL;
    double row[4], beta_pow[2];
    uint64_t steps = 0;
    double* theta = (double*)malloc(sizeof(double) * (size_t)np);
    CHECK(bsk_fit_stats_device(fit, &d_row));
    CHECK(bsk_fit_get_state(fit, theta, NULL, NULL, beta_pow, &steps));        /* (synchronises: the row is written) */
    if (hipMemcpy(row, d_row, sizeof row, 2)) return 3;
    printf("%a %a %a %a %a %a %a %a %a %a %a\n", row[0], row[1], row[2], row[3], theta[10], theta[11], theta[12], theta[13],
           (double)steps, beta_pow[0], beta_pow[1]);

    /* refusals */
    double target = 0.0;
    if (bsk_fit_accumulate(fit, d_obs, n, 0, d_labels, NULL, NULL, NULL, 0, NULL) != BSK_EINVAL) return 6;
    if (bsk_fit_accumulate(fit, d_obs, n, n, d_labels, &target, NULL, NULL, 0, NULL) != BSK_EINVAL) return 6;   /* no value network */
    if (bsk_fit_set_lr(fit, -1.0) != BSK_EINVAL || bsk_fit_step(NULL, NULL) != BSK_EINVAL) return 6;
    bsk_fit* refused = fit;
    if (bsk_fit_create(p, 1e-2, 1.0, 0.999, 1e-8, 0.0, 0.5, &refused) != BSK_EINVAL) return 7;
    if (refused != NULL) return 7;                   /* (a refused create leaves NULL) */
    bsk_fit_destroy(fit);
    if (hipFree(d_obs) || hipFree(d_labels)) return 3;
    bsk_policy_destroy(p);
    free(params); free(obs); free(labels); free(theta);
    return 0;
}
