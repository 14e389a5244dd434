/* Plain-C consumer of bsk_fork (include/bskgpu.h): a root batch is reset from the ICs in argv[1] and stepped under action 0, a branch
 * batch of three times its size forks every root env into three envs (branch j copies root j / 3), both step once more - the root under
 * action 0, branch j under action j % 3 - and a few numbers of both are printed.  The test compares them with the same calls through
 * the Python binding.  bsk_fork stages the host map itself: no device allocator is needed here. */
#include <stdio.h>
#include <stdlib.h>

#include "bskgpu.h"

#define CHECK(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, bsk_last_error()); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc < 3) return 9;
    const int n = atoi(argv[2]), nb = 3 * n, n_rw = 4;
    bsk_config cfg;
    CHECK(bsk_default_config(&cfg, n_rw, BSK_GRAV_PM_J2));
    bsk_handle *root = NULL, *branch = NULL;
    CHECK(bsk_create(&cfg, n, 0, NULL, &root));
    CHECK(bsk_create(&cfg, nb, 0, NULL, &branch));
    const int nf = bsk_n_fields(root);
    double* ic = (double*)calloc((size_t)nf * n, sizeof(double));
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(ic, sizeof(double), (size_t)nf * n, f) != (size_t)nf * n) { fprintf(stderr, "cannot read ICs\n"); return 4; }
    fclose(f);
    CHECK(bsk_reset(root, NULL, ic));
    int32_t* act = (int32_t*)calloc((size_t)nb, sizeof(int32_t));
    CHECK(bsk_step(root, act, 7));
    int32_t* map = (int32_t*)malloc(sizeof(int32_t) * nb);
    for (int j = 0; j < nb; ++j) map[j] = j / 3;
    CHECK(bsk_fork(branch, root, map));
    CHECK(bsk_step(root, act, 7));
    for (int j = 0; j < nb; ++j) act[j] = j % 3;
    CHECK(bsk_step(branch, act, 7));
    double* obs = (double*)malloc(sizeof(double) * 5 * nb);
    double* rew = (double*)malloc(sizeof(double) * nb);
    double* st = (double*)malloc(sizeof(double) * nf * nb);
    uint8_t* why = (uint8_t*)malloc(nb);
    int32_t* steps = (int32_t*)malloc(sizeof(int32_t) * nb);
    int32_t* ticks = (int32_t*)malloc(sizeof(int32_t) * nb);
    CHECK(bsk_get_obs_state(root, obs, rew, why, st));
    printf("%.17g %.17g %.17g ", obs[0], rew[n - 1], st[(size_t)9 * n + 1]);
    CHECK(bsk_get_obs_state(branch, obs, rew, why, st));
    CHECK(bsk_get_counters(branch, steps, ticks));
    double rsum = 0; int64_t ndone = 0;
    CHECK(bsk_get_batch_stats(branch, &rsum, &ndone));
    printf("%.17g %.17g %.17g %.17g %d %d %.17g %lld\n", obs[0], obs[2 * nb + 4], rew[nb - 1], st[(size_t)9 * nb + 5], steps[nb - 1],
           ticks[2], rsum, (long long)ndone);
    /* refusals: a NULL map, a partner of another config */
    if (bsk_fork(branch, root, NULL) != BSK_EINVAL) return 5;
    bsk_config other = cfg;
    other.dt = 0.05;
    bsk_handle* h2 = NULL;
    CHECK(bsk_create(&other, n, 0, NULL, &h2));
    if (bsk_fork(h2, root, map) != BSK_EINVAL) return 6;
    bsk_destroy(h2);
    bsk_destroy(branch);
    bsk_destroy(root);
    free(ic); free(act); free(map); free(obs); free(rew); free(st); free(why); free(steps); free(ticks);
    return 0;
}
