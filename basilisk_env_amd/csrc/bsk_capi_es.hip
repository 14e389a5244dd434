// bsk_capi_es.hip — C-ABI of the evolution strategy whose candidates never leave the device (bsk_es_*): ask into a population's
// parameter blocks, tell from a rollout's fitness, the optimiser and step-size rules, and the three records a tell keeps - the
// training log, the validation of the centre and the ring of episode outcomes.  Host side only, as bsk_capi.hip; kernels and launch wrappers: bsk_es.hip.
// The population and the observation statistics it reads through their handles: bsk_capi_policy.hpp.
#include <cmath>
#include <cstring>

#include "bsk_capi_policy.hpp"
#include "bsk_es.hpp"

using namespace bsk::capi;

namespace {

// The training log (bsk_es_set_log), the validation (bsk_es_set_validation) and the outcome ring (bsk_es_set_outcome_log) are one
// shape, a ring of per-generation rows and - the first two - a champion behind it, in ONE allocation of 8-byte words:
//   [head | gen C | row width * C | best_fitness | best_generation | best_member, - (log only) | cand | best_params ceil(n_params / 2)]
// head: the validation's V epoch words, none for the others; cand: the two ints the first launch of a record leaves for its
// second.  What is empty says so by the same sentinels in all: generation words all ones, a NaN fitness, zeroed parameters.
struct EsRecord {
    const int width;                       // doubles per row: 8 of the log, 4 of the validation, 3 * BSK_OUTCOME_COLS of the outcomes
    const int champion;                    // 8-byte words of the champion in front of its parameters: 4 with a member word
                                           // (started at -1; the log), 3 without (the validation), 0: the ring alone
    const char* const off;                 // what an accessor of a record that is off answers, behind its own name
    int head = 0, capacity = 0;            // capacity 0: off, and nothing below is there
    unsigned long long* d = nullptr;
    const double* d_src = nullptr;         // the caller's, bound by the setter: what the record's kernel reads beside the fitness -
                                           // the mean lengths (may be NULL), the outcome ring's member rows

    // the ring is the base shape of all three; the champion is a tail behind it whose length is formed here and nowhere else
    size_t tail_words(int n_params) const { return champion ? (size_t)champion + ((size_t)n_params + 1) / 2 : 0; }
    size_t words(int head_, int capacity_, int n_params) const {
        return (size_t)head_ + (size_t)(1 + width) * (size_t)capacity_ + tail_words(n_params);
    }
    unsigned long long* gen() const { return d + head; }
    double* row() const { return (double*)(gen() + capacity); }
    unsigned long long* tail() const { return gen() + (size_t)(1 + width) * (size_t)capacity; }
    double* best_fitness() const { return (double*)tail(); }
    unsigned long long* best_generation() const { return tail() + 1; }
    int* best_member() const { return (int*)(tail() + 2); }                   // (champion == 4 only)
    int* cand() const { return (int*)(tail() + champion - 1); }
    float* best_params() const { return (float*)(tail() + champion); }
};

}  // namespace

// bsk_es_*: the evolution strategy whose candidates never leave the device (bsk_es.hip)
struct bsk_es {
    bsk::PolicyLayout lay;
    int device = 0;
    int n_members = 0;
    double sigma = 0.0, lr = 0.0;
    int frozen = 0;
    unsigned long long* d_state = nullptr; // {seed, generation}: generation advanced behind every tell
    double* d_theta = nullptr;             // [lay.n_params]
    double* d_w = nullptr;                 // [w | q], n_members / 2 each: bsk_es_tell's scratch, the difference (and, under
                                           // BSK_ES_SIGMA_PGPE, the sum) of every pair's two utilities
    // bsk_es_set_optimizer: BSK_ES_SGD until Adam is selected; then ONE allocation [m | v | beta_pow] of 2 * n_params + 2 doubles
    int optimizer = BSK_ES_SGD;
    double beta1 = 0.0, beta2 = 0.0, eps = 0.0, weight_decay = 0.0;
    double* d_adam = nullptr;
    // bsk_es_set_sigma_adaptation: BSK_ES_SIGMA_FIXED until PGPE is selected; then sigma_vec [n_params]
    int sigma_kind = BSK_ES_SIGMA_FIXED;
    double lr_sigma = 0.0, max_change = 0.0, sigma_min = 0.0, sigma_max = 0.0;
    double* d_sigma = nullptr;
    // bsk_es_set_log: off until a capacity is given; then ONE allocation of 8-byte words
    // [log_gen C | log_row 8 C | best_fitness | best_generation | best_member, - | take, b | best_params ceil(n_params / 2)]
    EsRecord log = {8, 4, ": the optimiser has no log (bsk_es_set_log)"};
    hipStream_t last_stream = nullptr;     // of the last ask / tell / apply_obs_norm: what bsk_es_set_log asks about a capture
    // bsk_es_set_validation: off until n_val > 0; then ONE allocation of 8-byte words
    // [val_epoch V | val_gen C | val_row 4 C | val_best_fitness | val_best_generation | take, - | val_best_params ceil(n_params / 2)]
    // and d_src the caller's f64[n_members + n_val]
    EsRecord val = {4, 3, ": validation is off (bsk_es_set_validation)"};
    int n_val() const { return val.head; } // (the V epoch words are what stands in front of the validation's ring)
    // bsk_es_set_outcome_log: off until a capacity is given; then ONE allocation of 8-byte words [out_gen C | out_row 33 C], and
    // d_src the caller's member rows f64[n_members + n_val][BSK_OUTCOME_COLS]
    EsRecord outcome = {3 * BSK_OUTCOME_COLS, 0, ": the outcome ring is off (bsk_es_set_outcome_log)"};
};

namespace {

bsk::EsArgs es_args(const bsk_es* es) {
    bsk::EsArgs a;
    a.state = es->d_state;
    a.theta = es->d_theta;
    a.sigma = es->sigma;
    a.frozen = es->frozen;
    a.pairs = es->n_members / 2;
    return a;
}

bsk::EsAdam es_adam(const bsk_es* es) {
    const size_t np = (size_t)es->lay.n_params;
    bsk::EsAdam ad;
    ad.m = es->d_adam;
    ad.v = es->d_adam + np;
    ad.beta_pow = es->d_adam + 2 * np;
    ad.beta1 = es->beta1; ad.beta2 = es->beta2;
    ad.a1 = 1.0 - es->beta1; ad.a2 = 1.0 - es->beta2;
    ad.eps = es->eps; ad.weight_decay = es->weight_decay;
    ad.cg = 1.0 / ((double)es->n_members * es->sigma);
    ad.lr = es->lr;
    return ad;
}

bsk::EsSigma es_sigma(const bsk_es* es) {
    bsk::EsSigma sv;
    sv.sigma_vec = es->d_sigma;
    sv.pd = (double)es->n_members;
    sv.cs = es->lr_sigma / sv.pd;
    sv.max_change = es->max_change;
    sv.sigma_min = es->sigma_min;
    sv.sigma_max = es->sigma_max;
    return sv;
}

// the views of the two records the kernels take: what the two device structs share by name, then what each has of its own
template <class View>
View record_view(const EsRecord& r) {
    View v;
    v.gen = r.gen();
    v.row = r.row();
    v.best_fitness = r.best_fitness();
    v.best_generation = r.best_generation();
    v.cand = r.cand();
    v.best_params = r.best_params();
    v.mean_len = r.d_src;
    v.capacity = r.capacity;
    return v;
}

bsk::EsLog es_log(const bsk_es* es) {
    bsk::EsLog lg = record_view<bsk::EsLog>(es->log);
    lg.best_member = es->log.best_member();
    return lg;
}

bsk::EsVal es_val(const bsk_es* es) {
    bsk::EsVal vl = record_view<bsk::EsVal>(es->val);
    vl.n_val = es->val.head;
    return vl;
}

bsk::EsOutcome es_outcome(const bsk_es* es) {
    bsk::EsOutcome oc;
    oc.gen = es->outcome.gen();
    oc.row = es->outcome.row();
    oc.rows = es->outcome.d_src;
    oc.capacity = es->outcome.capacity;
    oc.n_val = es->n_val();
    return oc;
}

// (the optimiser serves one stream at a time: the stream of its last launch is the one a capture of its loop records)
bool es_stream_capturing(bsk_es* es) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (es->last_stream && hipStreamIsCapturing(es->last_stream, &st) != hipSuccess) {
        (void)hipGetLastError();                          // (a stream that has been destroyed since captures nothing)
        st = hipStreamCaptureStatusNone;
        es->last_stream = nullptr;
    }
    return st != hipStreamCaptureStatusNone;
}

// What both setters do first, with the device selected: refuse under capture before anything is freed, wait for the tells
// that are queued - they still write the old record - then free it and turn it off.
int record_off(bsk_es* es, EsRecord& r, const char* fn) {
    if (es_stream_capturing(es))
        return fail(BSK_EINVAL, std::string(fn) + ": the optimiser's stream is being captured; it allocates and synchronises and cannot be captured");
    HIP_SYNC(hipDeviceSynchronize());
    if (r.d) {
        (void)hipFree(r.d);
        r.d = nullptr;
    }
    r.head = r.capacity = 0;
    r.d_src = nullptr;
    return BSK_OK;
}

// ... and then, for a capacity: the allocation in its empty state - generation words all ones, rows, parameters and candidate
// words zero, the champion (where the record has one) a NaN of generation all ones (and member -1).  The head words are left to the caller, and so is
// turning the record on (head, capacity, d_src) once everything has succeeded.
int record_alloc(EsRecord& r, int head, int capacity, int n_params) {
    const size_t H = (size_t)head, C = (size_t)capacity, words = r.words(head, capacity, n_params);
    HIP_TRY(hipMalloc(&r.d, words * 8));
    HIP_TRY(hipMemset(r.d + H, 0xff, C * 8));
    HIP_TRY(hipMemset(r.d + H + C, 0, (words - H - C) * 8));
    const unsigned long long tail[3] = {0x7ff8000000000000ull, ~0ull, 0xffffffffull};
    if (r.champion) HIP_COPY(hipMemcpy(r.d + H + (size_t)(1 + r.width) * C, tail, (size_t)(r.champion - 1) * 8, hipMemcpyHostToDevice));
    return BSK_OK;
}

// what an accessor of a record that is off answers: composed here, from the entry point's name
int refuse_off(const EsRecord& r, const char* fn) { return fail(BSK_EINVAL, std::string(fn) + r.off); }

// what the accessors that copy refuse: `which` is &bsk_es::log or &bsk_es::val, fn the entry point's name
int record_check(const bsk_es* es, EsRecord bsk_es::*which, const char* fn) {
    if (!es) return fail(BSK_EINVAL, "es is NULL");
    return (es->*which).capacity < 1 ? refuse_off(es->*which, fn) : BSK_OK;
}

int record_get_rows(bsk_es* es, EsRecord bsk_es::*which, const char* fn, uint64_t* gen, double* rows) {
    if (int rc = record_check(es, which, fn)) return rc;
    const EsRecord& r = es->*which;
    const size_t C = (size_t)r.capacity;
    return transfer(es->device, hipMemcpyDeviceToHost, {{gen, r.gen(), C * 8}, {rows, r.row(), (size_t)r.width * C * 8}});
}

// the champion to the host or from it (member: NULL for the record that has none)
int record_champion(bsk_es* es, EsRecord bsk_es::*which, const char* fn, hipMemcpyKind dir, const float* params, const double* fitness,
                    const uint64_t* generation, const int32_t* member) {
    if (int rc = record_check(es, which, fn)) return rc;
    const EsRecord& r = es->*which;
    return transfer(es->device, dir, {{params, r.best_params(), (size_t)es->lay.n_params * sizeof(float)}, {fitness, r.best_fitness(), 8},
                                      {generation, r.best_generation(), 8}, {member, r.best_member(), 4}});
}

int record_best_device(bsk_es* es, EsRecord bsk_es::*which, const char* fn, const float** d_params) {
    if (!es || !d_params) return fail(BSK_EINVAL, "es/d_params is NULL");
    if ((es->*which).capacity < 1) return refuse_off(es->*which, fn);
    *d_params = (es->*which).best_params();
    return BSK_OK;
}

}  // namespace

extern "C" {

int bsk_es_create(const bsk_policy_spec* spec, int n_members, const float* theta, double sigma, double lr, int frozen, uint64_t seed,
                  int device_id, bsk_es** out) {
    bsk::PolicyLayout lay;
    int rc = create_begin(spec, out, lay);
    if (rc) return rc;
    if (n_members < 2 || n_members > 65536 || n_members % 2 != 0)
        return fail(BSK_EINVAL, "bsk_es_create: n_members must be even and in 2..65536 (the ranking compares every pair of members)");
    if (!std::isfinite(sigma) || !(sigma > 0.0)) return fail(BSK_EINVAL, "bsk_es_create: sigma must be finite and positive");
    if (!std::isfinite(lr)) return fail(BSK_EINVAL, "bsk_es_create: lr must be finite");
    if (frozen < 0 || frozen > lay.n_params) return fail(BSK_EINVAL, "bsk_es_create: frozen must be in 0..n_params");
    return create_on_device(lay, device_id, out, bsk_es_destroy, [&](bsk_es* es) -> int {
        es->n_members = n_members;
        es->sigma = sigma;
        es->lr = lr;
        es->frozen = frozen;
        const unsigned long long state0[2] = {seed, 0ull};
        std::vector<double> theta0((size_t)lay.n_params, 0.0);
        if (theta)
            for (int j = 0; j < lay.n_params; ++j) theta0[(size_t)j] = (double)theta[j];
        HIP_TRY(hipMalloc(&es->d_state, sizeof state0));
        HIP_TRY(hipMalloc(&es->d_theta, theta0.size() * sizeof(double)));
        HIP_TRY(hipMalloc(&es->d_w, (size_t)n_members * sizeof(double)));
        HIP_COPY(hipMemcpy(es->d_state, state0, sizeof state0, hipMemcpyHostToDevice));
        HIP_COPY(hipMemcpy(es->d_theta, theta0.data(), theta0.size() * sizeof(double), hipMemcpyHostToDevice));
        return BSK_OK;
    });
}

void bsk_es_destroy(bsk_es* es) {
    if (!es) return;
    DeviceGuard guard(es->device);
    free_all({es->d_state, es->d_theta, es->d_w, es->d_adam, es->d_sigma, es->log.d, es->val.d, es->outcome.d});
    delete es;
}

int bsk_es_ask(bsk_es* es, bsk_population* pop, void* stream) {
    if (!es || !pop) return fail(BSK_EINVAL, "es/population is NULL");
    if (pop->n_members != es->n_members + es->n_val())
        return fail(BSK_EINVAL, es->n_val() > 0 ? "bsk_es_ask: the population's n_members differs from the optimiser's n_members + n_val (bsk_es_set_validation)"
                                                : "bsk_es_ask: the population's n_members differs from the optimiser's");
    if (std::memcmp(&pop->lay, &es->lay, sizeof(bsk::PolicyLayout)) != 0)      // (all-int, value-initialised: policy_layout)
        return fail(BSK_EINVAL, "bsk_es_ask: the population's spec differs from the optimiser's");
    if (pop->device != es->device) return fail(BSK_EINVAL, "bsk_es_ask: the optimiser and the population live on different devices");
    DeviceGuard guard(es->device);
    es->last_stream = (hipStream_t)stream;
    if (es->sigma_kind == BSK_ES_SIGMA_PGPE)
        HIP_TRY(bsk::launch_es_ask_sigma(es->lay, es_args(es), es->d_sigma, pop->d_params, (hipStream_t)stream));
    else
        HIP_TRY(bsk::launch_es_ask(es->lay, es_args(es), pop->d_params, (hipStream_t)stream));
    if (es->n_val() > 0)                                  // the centre into the members behind ask's: member-major, so the launch above is the one it was
        HIP_TRY(bsk::launch_es_center(es->lay, es->d_theta, pop->d_params + (size_t)es->n_members * (size_t)es->lay.n_device, es->n_val(),
                                      (hipStream_t)stream));
    return BSK_OK;        // asynchronous on `stream`: no copy, no synchronisation
}

int bsk_es_tell(bsk_es* es, const double* d_fitness, void* stream) {
    if (!es || !d_fitness) return fail(BSK_EINVAL, "es/d_fitness is NULL");
    DeviceGuard guard(es->device);
    const hipStream_t s = (hipStream_t)stream;
    const bool adam = es->optimizer == BSK_ES_ADAM, pgpe = es->sigma_kind == BSK_ES_SIGMA_PGPE;
    const int P = es->n_members, np = es->lay.n_params;
    const bsk::EsArgs a = es_args(es);
    double *d_w = es->d_w, *d_q = es->d_w + P / 2;
    es->last_stream = s;
    // the log, in front of the update: theta, sigma_vec and the generation as ask read them
    if (es->log.capacity > 0) HIP_TRY(bsk::launch_es_log(a, pgpe ? es->d_sigma : nullptr, np, d_fitness, es_log(es), s));
    // the validation, behind the log's two launches and in front of the update too: f[P .. P + V - 1]
    if (es->n_val() > 0) HIP_TRY(bsk::launch_es_validate(a, np, d_fitness, es_val(es), s));
    // the outcome ring, in front of the update too: its own launch, reading the member rows the rollout left
    if (es->outcome.capacity > 0) HIP_TRY(bsk::launch_es_outcome(a, d_fitness, es_outcome(es), s));
    // the ranking of the first P; a step size per parameter wants the sum of every pair's utilities beside their difference
    if (pgpe) HIP_TRY(bsk::launch_es_rank_q(d_fitness, P, d_w, d_q, s));
    else      HIP_TRY(bsk::launch_es_rank(d_fitness, P, d_w, s));
    // the update: optimiser x sigma kind
    if (adam && pgpe)  HIP_TRY(bsk::launch_es_tell_adam_sigma(a, np, d_w, d_q, es_adam(es), es_sigma(es), s));
    else if (adam)     HIP_TRY(bsk::launch_es_tell_adam(a, np, d_w, es_adam(es), s));
    else if (pgpe)     HIP_TRY(bsk::launch_es_tell_sigma(a, np, d_w, d_q, es->lr, es_sigma(es), s));
    else               HIP_TRY(bsk::launch_es_tell(a, np, d_w, es->lr / ((double)P * es->sigma), s));
    // the generation word moves on, and Adam's running powers with it
    if (adam) HIP_TRY(bsk::launch_es_advance_adam(es->d_state, es->d_adam + 2 * (size_t)np, es->beta1, es->beta2, s));
    else      HIP_TRY(bsk::launch_es_advance(es->d_state, s));
    return BSK_OK;
}

int bsk_es_get_state(bsk_es* es, double* theta, uint64_t* generation) {
    if (!es) return fail(BSK_EINVAL, "es is NULL");
    unsigned long long w[2];                              // {seed, generation}: read as the pair they are
    int rc = transfer(es->device, hipMemcpyDeviceToHost, {{theta, es->d_theta, (size_t)es->lay.n_params * sizeof(double)},
                                                          {generation ? w : nullptr, es->d_state, sizeof w}});
    if (rc == BSK_OK && generation) *generation = w[1];
    return rc;
}

int bsk_es_set_state(bsk_es* es, const double* theta, uint64_t generation) {
    if (!es) return fail(BSK_EINVAL, "es is NULL");
    const unsigned long long g = generation;
    return transfer(es->device, hipMemcpyHostToDevice, {{theta, es->d_theta, (size_t)es->lay.n_params * sizeof(double)},
                                                        {&g, es->d_state + 1, sizeof g}});
}

int bsk_es_generation_device(bsk_es* es, const uint64_t** d_generation) {
    if (!es || !d_generation) return fail(BSK_EINVAL, "es/d_generation is NULL");
    *d_generation = (const uint64_t*)(es->d_state + 1);
    return BSK_OK;
}

int bsk_es_set_optimizer(bsk_es* es, int kind, double beta1, double beta2, double eps, double weight_decay) {
    if (!es) return fail(BSK_EINVAL, "es is NULL");
    if (kind != BSK_ES_SGD && kind != BSK_ES_ADAM) return fail(BSK_EINVAL, "bsk_es_set_optimizer: kind must be BSK_ES_SGD or BSK_ES_ADAM");
    if (kind == BSK_ES_ADAM) {
        if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
            return fail(BSK_EINVAL, "bsk_es_set_optimizer: beta1 and beta2 must be in [0, 1)");
        if (!std::isfinite(eps) || !(eps > 0.0)) return fail(BSK_EINVAL, "bsk_es_set_optimizer: eps must be finite and positive");
        if (!std::isfinite(weight_decay) || weight_decay < 0.0)
            return fail(BSK_EINVAL, "bsk_es_set_optimizer: weight_decay must be finite and not negative");
    }
    DeviceGuard guard(es->device);
    HIP_SYNC(hipDeviceSynchronize());                     // (queued tells still use the old rule and the old moments)
    if (kind == BSK_ES_SGD) {
        es->optimizer = BSK_ES_SGD;
        return BSK_OK;
    }
    const size_t np = (size_t)es->lay.n_params;
    if (!es->d_adam) HIP_TRY(hipMalloc(&es->d_adam, (2 * np + 2) * sizeof(double)));
    const double one[2] = {1.0, 1.0};
    HIP_TRY(hipMemset(es->d_adam, 0, 2 * np * sizeof(double)));
    HIP_COPY(hipMemcpy(es->d_adam + 2 * np, one, sizeof one, hipMemcpyHostToDevice));
    es->optimizer = BSK_ES_ADAM;
    es->beta1 = beta1; es->beta2 = beta2; es->eps = eps; es->weight_decay = weight_decay;
    return BSK_OK;
}

// Adam's [m | v | beta_pow] to the host or from it
static int es_moments(bsk_es* es, const char* fn, hipMemcpyKind dir, const double* m, const double* v, const double* beta_pow) {
    if (!es) return fail(BSK_EINVAL, "es is NULL");
    if (es->optimizer != BSK_ES_ADAM) return fail(BSK_EINVAL, std::string(fn) + ": the optimiser is BSK_ES_SGD, it has no moments");
    const size_t np = (size_t)es->lay.n_params;
    return transfer(es->device, dir, {{m, es->d_adam, np * sizeof(double)}, {v, es->d_adam + np, np * sizeof(double)},
                                      {beta_pow, es->d_adam + 2 * np, 2 * sizeof(double)}});
}
int bsk_es_get_moments(bsk_es* es, double* m, double* v, double* beta_pow) {
    return es_moments(es, "bsk_es_get_moments", hipMemcpyDeviceToHost, m, v, beta_pow);
}
int bsk_es_set_moments(bsk_es* es, const double* m, const double* v, const double* beta_pow) {
    return es_moments(es, "bsk_es_set_moments", hipMemcpyHostToDevice, m, v, beta_pow);
}

int bsk_es_set_sigma_adaptation(bsk_es* es, int kind, double lr_sigma, double max_change, double sigma_min, double sigma_max) {
    const char* const fn = "bsk_es_set_sigma_adaptation: ";
    if (!es) return fail(BSK_EINVAL, "es is NULL");
    if (kind != BSK_ES_SIGMA_FIXED && kind != BSK_ES_SIGMA_PGPE)
        return fail(BSK_EINVAL, std::string(fn) + "kind must be BSK_ES_SIGMA_FIXED or BSK_ES_SIGMA_PGPE");
    if (kind == BSK_ES_SIGMA_PGPE) {
        if (!std::isfinite(lr_sigma) || lr_sigma < 0.0) return fail(BSK_EINVAL, std::string(fn) + "lr_sigma must be finite and not negative");
        if (!std::isfinite(max_change) || !(max_change > 0.0 && max_change < 1.0))
            return fail(BSK_EINVAL, std::string(fn) + "max_change must be inside (0, 1)");
        if (!std::isfinite(sigma_min) || !(sigma_min > 0.0)) return fail(BSK_EINVAL, std::string(fn) + "sigma_min must be finite and positive");
        if (!std::isfinite(sigma_max) || sigma_max < sigma_min)
            return fail(BSK_EINVAL, std::string(fn) + "sigma_max must be finite and not below sigma_min");
        if (es->sigma < sigma_min || es->sigma > sigma_max)
            return fail(BSK_EINVAL, std::string(fn) + "the sigma of bsk_es_create must be inside [sigma_min, sigma_max]");
    }
    DeviceGuard guard(es->device);
    HIP_SYNC(hipDeviceSynchronize());                     // (queued asks and tells still use the old rule and the old vector)
    if (kind == BSK_ES_SIGMA_FIXED) {
        es->sigma_kind = BSK_ES_SIGMA_FIXED;
        return BSK_OK;
    }
    const size_t np = (size_t)es->lay.n_params;
    if (!es->d_sigma) HIP_TRY(hipMalloc(&es->d_sigma, np * sizeof(double)));
    const std::vector<double> fill(np, es->sigma);
    HIP_COPY(hipMemcpy(es->d_sigma, fill.data(), np * sizeof(double), hipMemcpyHostToDevice));
    es->sigma_kind = BSK_ES_SIGMA_PGPE;
    es->lr_sigma = lr_sigma; es->max_change = max_change; es->sigma_min = sigma_min; es->sigma_max = sigma_max;
    return BSK_OK;
}

// what both accessors of sigma_vec refuse
static int es_sigma_check(const bsk_es* es, const char* fn, const double* sigma) {
    if (!es || !sigma) return fail(BSK_EINVAL, "es/sigma is NULL");
    if (es->sigma_kind != BSK_ES_SIGMA_PGPE) return fail(BSK_EINVAL, std::string(fn) + ": the kind is BSK_ES_SIGMA_FIXED, there is no vector");
    return BSK_OK;
}
int bsk_es_get_sigma(bsk_es* es, double* sigma) {
    if (int rc = es_sigma_check(es, "bsk_es_get_sigma", sigma)) return rc;
    return transfer(es->device, hipMemcpyDeviceToHost, {{sigma, es->d_sigma, (size_t)es->lay.n_params * sizeof(double)}});
}
int bsk_es_set_sigma(bsk_es* es, const double* sigma) {
    if (int rc = es_sigma_check(es, "bsk_es_set_sigma", sigma)) return rc;
    for (int j = 0; j < es->lay.n_params; ++j)
        if (!std::isfinite(sigma[j]) || !(sigma[j] > 0.0)) return fail(BSK_EINVAL, "bsk_es_set_sigma: every entry must be finite and positive");
    return transfer(es->device, hipMemcpyHostToDevice, {{sigma, es->d_sigma, (size_t)es->lay.n_params * sizeof(double)}});
}

int bsk_es_set_log(bsk_es* es, int capacity, const double* d_mean_len) {
    if (!es) return fail(BSK_EINVAL, "es is NULL");
    if (capacity < 0) return fail(BSK_EINVAL, "bsk_es_set_log: capacity must not be negative");
    DeviceGuard guard(es->device);
    int rc = record_off(es, es->log, "bsk_es_set_log");
    if (rc || capacity == 0) return rc;
    if ((rc = record_alloc(es->log, 0, capacity, es->lay.n_params))) return rc;
    es->log.capacity = capacity;
    es->log.d_src = d_mean_len;
    return BSK_OK;
}

int bsk_es_set_validation(bsk_es* es, int n_val, int capacity, uint64_t epoch0, const double* d_mean_len) {
    if (!es) return fail(BSK_EINVAL, "es is NULL");
    if (n_val < 0 || n_val > 16) return fail(BSK_EINVAL, "bsk_es_set_validation: n_val must be in 0..16");
    if (n_val > 0 && capacity < 1) return fail(BSK_EINVAL, "bsk_es_set_validation: capacity must be >= 1");
    DeviceGuard guard(es->device);
    int rc = record_off(es, es->val, "bsk_es_set_validation");
    if (rc || n_val == 0) return rc;
    if ((rc = record_alloc(es->val, n_val, capacity, es->lay.n_params))) return rc;
    std::vector<unsigned long long> epochs((size_t)n_val);                  // val_epoch: its own, in front of the ring
    for (int v = 0; v < n_val; ++v) epochs[(size_t)v] = epoch0 + (unsigned long long)v;
    HIP_COPY(hipMemcpy(es->val.d, epochs.data(), epochs.size() * 8, hipMemcpyHostToDevice));
    HIP_SYNC(hipDeviceSynchronize());                     // (its own too: the caller's next reset reads the epoch words from any stream)
    es->val.head = n_val;
    es->val.capacity = capacity;
    es->val.d_src = d_mean_len;
    return BSK_OK;
}

int bsk_es_set_outcome_log(bsk_es* es, int capacity, const double* d_rows) {
    if (!es) return fail(BSK_EINVAL, "es is NULL");
    if (capacity < 0) return fail(BSK_EINVAL, "bsk_es_set_outcome_log: capacity must not be negative");
    if (capacity > 0 && !d_rows) return fail(BSK_EINVAL, "bsk_es_set_outcome_log: d_rows is NULL");
    DeviceGuard guard(es->device);
    int rc = record_off(es, es->outcome, "bsk_es_set_outcome_log");
    if (rc || capacity == 0) return rc;
    if ((rc = record_alloc(es->outcome, 0, capacity, 0))) return rc;        // (no champion: no parameters to hold)
    es->outcome.capacity = capacity;
    es->outcome.d_src = d_rows;
    return BSK_OK;
}

int bsk_es_get_outcome_log(bsk_es* es, uint64_t* gen, double* rows) {
    return record_get_rows(es, &bsk_es::outcome, "bsk_es_get_outcome_log", gen, rows);
}
int bsk_es_get_log(bsk_es* es, uint64_t* gen, double* rows) { return record_get_rows(es, &bsk_es::log, "bsk_es_get_log", gen, rows); }
int bsk_es_get_validation_log(bsk_es* es, uint64_t* gen, double* rows) {
    return record_get_rows(es, &bsk_es::val, "bsk_es_get_validation_log", gen, rows);
}

int bsk_es_get_best(bsk_es* es, float* params, double* fitness, uint64_t* generation, int32_t* member) {
    return record_champion(es, &bsk_es::log, "bsk_es_get_best", hipMemcpyDeviceToHost, params, fitness, generation, member);
}
int bsk_es_set_best(bsk_es* es, const float* params, const double* fitness, const uint64_t* generation, const int32_t* member) {
    return record_champion(es, &bsk_es::log, "bsk_es_set_best", hipMemcpyHostToDevice, params, fitness, generation, member);
}
int bsk_es_get_validated_best(bsk_es* es, float* params, double* fitness, uint64_t* generation) {
    return record_champion(es, &bsk_es::val, "bsk_es_get_validated_best", hipMemcpyDeviceToHost, params, fitness, generation, nullptr);
}
int bsk_es_set_validated_best(bsk_es* es, const float* params, const double* fitness, const uint64_t* generation) {
    return record_champion(es, &bsk_es::val, "bsk_es_set_validated_best", hipMemcpyHostToDevice, params, fitness, generation, nullptr);
}

int bsk_es_best_device(bsk_es* es, const float** d_params) { return record_best_device(es, &bsk_es::log, "bsk_es_best_device", d_params); }
int bsk_es_validated_best_device(bsk_es* es, const float** d_params) {
    return record_best_device(es, &bsk_es::val, "bsk_es_validated_best_device", d_params);
}

int bsk_es_validation_epochs_device(bsk_es* es, const uint64_t** d_epochs) {
    if (!es || !d_epochs) return fail(BSK_EINVAL, "es/d_epochs is NULL");
    if (es->val.capacity < 1) return refuse_off(es->val, "bsk_es_validation_epochs_device");
    *d_epochs = (const uint64_t*)es->val.d;
    return BSK_OK;
}

int bsk_es_apply_obs_norm(bsk_es* es, bsk_obs_stats* s, double std_min, void* stream) {
    if (!es || !s) return fail(BSK_EINVAL, "es/stats is NULL");
    if (es->frozen < 10)
        return fail(BSK_EINVAL, "bsk_es_apply_obs_norm: frozen must be >= 10 (in_scale and in_shift would be perturbed and moved by the search)");
    if (!std::isfinite(std_min) || !(std_min > 0.0)) return fail(BSK_EINVAL, "bsk_es_apply_obs_norm: std_min must be finite and positive");
    if (es->device != s->device) return fail(BSK_EINVAL, "bsk_es_apply_obs_norm: the optimiser and the statistics live on different devices");
    DeviceGuard guard(es->device);
    es->last_stream = (hipStream_t)stream;
    HIP_TRY(bsk::launch_es_obs_norm(s->st.tot, s->st.tot_n, std_min, es->d_theta, (hipStream_t)stream));
    return BSK_OK;        // asynchronous on `stream`: no copy, no synchronisation
}
}  // extern "C"
