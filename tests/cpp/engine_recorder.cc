// engine_recorder.cc - a recording stand-in for the engine: exactly the functions of include/fabber_vb.h that the host
// library (fabber_core_amd/csrc/host) calls. Every call writes a text record of what it was handed - contents, never
// addresses - fills the outputs with a scripted, valid result and returns a scripted code. Linked with the host sources
// instead of the engine, it shows which entry point a run takes and with which fvb_config, without a GPU
// (tests/test_engine_routing.py).
#include "engine_recorder.h"

#include "../../include/fabber_vb.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>

EngineScript engine_script;
// the lines of the first fvb_config record of all, and of the record that the next one is compared with: the scenario's
// previous one, or at its start the first of all
static std::vector<std::string> first_config, last_config;
static const char *last_config_name = "";

void engine_record(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vprintf(fmt, ap);
    va_end(ap);
    putchar('\n');
}

void engine_begin_scenario(const char *title)
{
    engine_record("==== %s", title);
    engine_script = EngineScript();
    last_config = first_config;
    last_config_name = "the first record of all";
}

namespace
{
std::string text(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
std::string text(const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return buf;
}
// " name v v v": the values in full (%.17g), a run of equal values as "v xN"; " name NULL" without an array
template <typename T> std::string values(const char *name, const T *p, size_t n, const char *fmt)
{
    std::string out = std::string(" ") + name;
    if (!p)
        return out + " NULL";
    for (size_t i = 0, j; i < n; i = j)
    {
        for (j = i + 1; j < n && p[j] == p[i]; j++)
        {
        }
        out += " " + text(fmt, p[i]) + (j - i > 1 ? text(" x%d", (int)(j - i)) : std::string());
    }
    return out;
}
std::string doubles(const char *name, const double *p, size_t n)
{
    return values(name, p, n, "%.17g");
}
template <typename T> std::string ints(const char *name, const T *p, size_t n)
{
    std::vector<int> wide(p ? p : NULL, p ? p + n : NULL);
    return values(name, p ? wide.data() : NULL, n, "%d");
}
int noise_entries(const fvb_config *c)
{
    return (c->noise == FVB_NOISE_AR1 ? 2 + c->ar_cross_terms : 0) + c->n_phis;
}
int mvn_rows(int n)
{
    return n * (n + 1) / 2 + n + 1;
}

// Every scalar of the block and the contents of everything it points to, as a fixed list of lines. The first record of
// all prints them all; a later one prints the lines that differ from the scenario's record before it, and the first of a
// scenario those that differ from the first record of all.
void put_config(const fvb_config *c)
{
    const int P = c->n_params, V = c->n_voxels, T = c->n_times;
    const fvb_param_table *x = c->params_ext;
    std::vector<std::string> l;
    l.push_back(text("abi_version=%d n_voxels=%d n_times=%d n_params=%d n_phis=%d noise=%d", c->abi_version, V, T, P, c->n_phis, c->noise));
    l.push_back(text("model=%d device_model='%s'", c->model, c->device_model) + ints("model_iopt", c->model_iopt, 4) + doubles("model_dopt", c->model_dopt, 4));
    l.push_back(doubles("design", c->design, (size_t)T * P));
    l.push_back(std::string("parameters from the ") + (x ? "table (params_ext):" : "struct:") + ints("transform", x ? x->transform : c->transform, P)
        + ints("prior_type", x ? x->prior_type : c->prior_type, P));
    l.push_back(doubles("prior_mean", x ? x->prior_mean : c->prior_mean, P) + doubles("prior_var", x ? x->prior_var : c->prior_var, P)
        + doubles("prior_prec", x ? x->prior_prec : c->prior_prec, P));
    l.push_back(doubles("post_mean", x ? x->post_mean : c->post_mean, P) + doubles("post_var", x ? x->post_var : c->post_var, P));
    std::string images = "image priors:";
    for (int k = 0; k < P; k++)
        if (const double *img = x ? x->image_prior[k] : c->image_prior[k])
            images += doubles(text("[%d]", k).c_str(), img, V);
    l.push_back(images);
    l.push_back(doubles("noise_prior_b", c->noise_prior_b, FVB_MAX_PHIS) + doubles("noise_prior_c", c->noise_prior_c, FVB_MAX_PHIS)
        + doubles("noise_post_b", c->noise_post_b, FVB_MAX_PHIS) + doubles("noise_post_c", c->noise_post_c, FVB_MAX_PHIS)
        + text(" locked_noise_stdev=%.17g", c->locked_noise_stdev));
    l.push_back(ints("phi_index", c->phi_index, T));
    l.push_back(text("convergence=%d max_iterations=%d max_trials=%d need_f=%d min_fchange=%.17g f_history_rows=%d data_f64=%d", c->convergence,
        c->max_iterations, c->max_trials, c->need_f, c->min_fchange, c->f_history_rows, c->data_f64));
    l.push_back(doubles("init_mvn", c->init_mvn, (size_t)mvn_rows(P + noise_entries(c)) * V));
    l.push_back(text("ar_cross_terms=%d ar_alpha_given=%d", c->ar_cross_terms, c->ar_alpha_given) + doubles("prior_mean", c->ar_alpha_prior_mean, FVB_MAX_ALPHAS)
        + doubles("prior_prec", &c->ar_alpha_prior_prec[0][0], FVB_MAX_ALPHAS * FVB_MAX_ALPHAS) + doubles("post_mean", c->ar_alpha_post_mean, FVB_MAX_ALPHAS)
        + doubles("post_cov", &c->ar_alpha_post_cov[0][0], FVB_MAX_ALPHAS * FVB_MAX_ALPHAS));
    l.push_back(text("n_model_consts=%d", c->n_model_consts) + doubles("model_consts", c->model_consts, c->n_model_consts)
        + text(" n_model_supp=%d", c->n_model_supp) + doubles("model_supp", c->model_supp, (size_t)c->n_model_supp * V));
    if (!last_config.empty())
        printf("  cfg as in %s%s\n", last_config_name, l == last_config ? "" : ", but for:");
    for (size_t i = 0; i < l.size(); i++)
        if (last_config.empty() || l[i] != last_config[i])
            printf("  cfg %s\n", l[i].c_str());
    if (first_config.empty())
        first_config = l;
    last_config = l;
    last_config_name = "the record before";
}

void put_series(const fvb_config *c, const void *data)
{
    const size_t n = (size_t)c->n_times * c->n_voxels;
    if (!data || n == 0)
        printf("  series NULL\n");
    else if (c->data_f64) // (the store of the run data's NEWMAT::Matrix, timepoints x voxels)
        printf("  series float64 matrix %d x %d first=%.17g last=%.17g\n", c->n_times, c->n_voxels, ((const double *)data)[0],
            ((const double *)data)[n - 1]);
    else
        printf("  series float32 first=%.17g last=%.17g\n", (double)((const float *)data)[0], (double)((const float *)data)[n - 1]);
}

void put_spatial(const fvb_config *c, const fvb_spatial *sp)
{
    printf("  spatial dims=%d update_first_iter=%d speed=%.17g q1=%.17g q2=%.17g owned=[%d,%d) n_voxels_global=%d%s\n", sp->spatial_dims,
        sp->update_first_iter, sp->spatial_speed, sp->q1, sp->q2, sp->owned_begin, sp->owned_end, sp->n_voxels_global,
        ints("coords", sp->coords, (size_t)3 * c->n_voxels).c_str());
    printf(" %s\n", doubles("locked_centres", sp->locked_centres, (size_t)c->n_params * c->n_voxels).c_str());
}

void put_devices(const int32_t *devices, int32_t n)
{
    printf("  n_devices=%d%s\n", n, ints("devices", devices, n).c_str());
}

// the scripted, valid result: unit covariance, means 1, 2, ..., last row 1
int fill_outputs(const fvb_config *c, const fvb_outputs *out, int rc)
{
    const int V = c->n_voxels, n = c->n_params + noise_entries(c), nCov = n * (n + 1) / 2;
    printf("  outputs set:%s%s%s%s%s%s -> %d\n", out->mvn ? " mvn" : "", out->free_energy ? " free_energy" : "", out->f_history ? " f_history" : "",
        out->f_history_len ? " f_history_len" : "", out->status ? " status" : "", out->iterations ? " iterations" : "", rc);
    for (int v = 0; v < V; v++)
    {
        for (int r = 0; r < mvn_rows(n); r++)
            out->mvn[(size_t)r * V + v] = 0;
        for (int i = 0; i < n; i++)
        {
            out->mvn[(size_t)(i * (i + 1) / 2 + i) * V + v] = 1;
            out->mvn[(size_t)(nCov + i) * V + v] = i + 1;
        }
        out->mvn[(size_t)(nCov + n) * V + v] = 1;
        if (out->free_energy)
            out->free_energy[v] = -(v + 1);
        if (out->status)
            out->status[v] = v < (int)engine_script.status.size() ? engine_script.status[v] : 0;
        if (out->iterations)
            out->iterations[v] = v + 1;
        if (out->f_history_len)
            out->f_history_len[v] = v < (int)engine_script.hist_len.size() ? engine_script.hist_len[v] : c->f_history_rows;
        for (int r = 0; out->f_history && r < c->f_history_rows; r++)
            out->f_history[(size_t)r * V + v] = 100 * v + r;
    }
    return rc;
}

// the model's host code, once about the starting estimate of every voxel
void call_linearise(const fvb_config *c, fvb_linearise_fn linearise, void *user)
{
    const int V = c->n_voxels, P = c->n_params, T = c->n_times;
    std::vector<int32_t> ids(V);
    std::vector<double> means((size_t)V * P), lin((size_t)V * T * (P + 1), 0.0);
    for (int v = 0; v < V; v++)
    {
        ids[v] = v;
        for (int k = 0; k < P; k++)
            means[(size_t)v * P + k] = FVB_PARAM(c, post_mean, k);
    }
    const int rc = linearise(user, V, ids.data(), means.data(), lin.data());
    double sum = 0;
    for (size_t i = 0; i < lin.size(); i++)
        sum += lin[i];
    printf("  linearise -> %d, offsets and jacobians: first=%.17g last=%.17g sum=%.17g\n", rc, lin.front(), lin.back(), sum);
}

bool is_plugin(const fvb_config *c)
{
    return c->model == FVB_MODEL_PLUGIN;
}
} // namespace

extern "C" {
int32_t fabber_vb_mvn_rows(int32_t n)
{
    engine_record("fabber_vb_mvn_rows n=%d", n);
    return mvn_rows(n);
}
const char *fabber_vb_last_error(void)
{
    engine_record("fabber_vb_last_error");
    return "the recorder's error text";
}
void fabber_vb_trim_cached_memory(uint64_t keep_bytes)
{
    engine_record("fabber_vb_trim_cached_memory keep_bytes=%llu", (unsigned long long)keep_bytes);
}
int32_t fabber_vb_device_model_count(void)
{
    engine_record("fabber_vb_device_model_count -> %d", (int)engine_script.device_models.size());
    return (int32_t)engine_script.device_models.size();
}
const char *fabber_vb_device_model_name(int32_t i)
{
    const char *name = i >= 0 && i < (int)engine_script.device_models.size() ? engine_script.device_models[i].c_str() : NULL;
    engine_record("fabber_vb_device_model_name i=%d -> %s", i, name ? name : "NULL");
    return name;
}

static const char *kernel_name(const char *fn, const fvb_config *cfg, const char *answer)
{
    engine_record("%s", fn);
    put_config(cfg);
    printf("  -> '%s'\n", answer);
    return answer;
}
const char *fabber_vb_kernel_name(const fvb_config *cfg)
{
    return kernel_name("fabber_vb_kernel_name", cfg, "recorded");
}
const char *fabber_vb_init_posterior_kernel_name(const fvb_config *cfg)
{
    return kernel_name("fabber_vb_init_posterior_kernel_name", cfg, is_plugin(cfg) && !cfg->init_mvn ? engine_script.init_kernel.c_str() : "");
}
const char *fabber_vb_spatial_kernel_name(const fvb_config *cfg)
{
    return kernel_name("fabber_vb_spatial_kernel_name", cfg, is_plugin(cfg) ? engine_script.spatial_kernel.c_str() : "");
}
const char *fabber_vb_postproc_kernel_name(const fvb_config *cfg)
{
    return kernel_name("fabber_vb_postproc_kernel_name", cfg, is_plugin(cfg) ? engine_script.postproc_kernel.c_str() : "postproc");
}
const char *fabber_nlls_kernel_name(const fvb_config *cfg)
{
    return kernel_name("fabber_nlls_kernel_name", cfg, is_plugin(cfg) ? engine_script.nlls_kernel.c_str() : "nlls");
}

int32_t fabber_vb_run_host(const fvb_config *cfg, const void *data, const fvb_outputs *out, int32_t device)
{
    engine_record("fabber_vb_run_host device=%d", device);
    put_config(cfg);
    put_series(cfg, data);
    return fill_outputs(cfg, out, 0);
}
int32_t fabber_vb_run_host_multi(const fvb_config *cfg, const void *data, const fvb_outputs *out, const int32_t *devices, int32_t n_devices,
    fvb_summary *summary)
{
    engine_record("fabber_vb_run_host_multi summary %s", summary ? "set" : "NULL");
    put_devices(devices, n_devices);
    put_config(cfg);
    put_series(cfg, data);
    if (summary)
    {
        summary->sum_free_energy = -21;
        summary->sum_iterations = 21;
        summary->bad_voxels = 0;
    }
    return fill_outputs(cfg, out, 0);
}
int32_t fabber_vb_run_hostmodel_host(const fvb_config *cfg, const void *data, const fvb_outputs *out, int32_t device, fvb_linearise_fn linearise,
    void *user)
{
    engine_record("fabber_vb_run_hostmodel_host device=%d", device);
    put_config(cfg);
    put_series(cfg, data);
    call_linearise(cfg, linearise, user);
    return fill_outputs(cfg, out, 0);
}
int32_t fabber_vb_run_spatial_host(const fvb_config *cfg, const fvb_spatial *sp, const void *data, const fvb_outputs *out, int32_t device,
    void (*progress_cb)(int, int))
{
    engine_record("fabber_vb_run_spatial_host device=%d", device);
    put_config(cfg);
    put_spatial(cfg, sp);
    put_series(cfg, data);
    if (engine_script.rc_spatial_host != 0)
    {
        printf("  -> %d\n", engine_script.rc_spatial_host);
        return engine_script.rc_spatial_host;
    }
    if (progress_cb)
        progress_cb(1, cfg->max_iterations);
    return fill_outputs(cfg, out, 0);
}
int32_t fabber_vb_run_spatial_host_multi(const fvb_config *cfg, const fvb_spatial *sp, const void *data, const fvb_outputs *out,
    const int32_t *devices, int32_t n_devices, void (*progress_cb)(int, int))
{
    engine_record("fabber_vb_run_spatial_host_multi");
    put_devices(devices, n_devices);
    put_config(cfg);
    put_spatial(cfg, sp);
    put_series(cfg, data);
    if (progress_cb)
        progress_cb(1, cfg->max_iterations);
    return fill_outputs(cfg, out, 0);
}
int32_t fabber_vb_run_spatial_hostmodel_host(const fvb_config *cfg, const fvb_spatial *sp, const void *data, const fvb_outputs *out,
    int32_t device, fvb_linearise_fn linearise, void *user, void (*progress_cb)(int, int))
{
    engine_record("fabber_vb_run_spatial_hostmodel_host device=%d", device);
    put_config(cfg);
    put_spatial(cfg, sp);
    put_series(cfg, data);
    call_linearise(cfg, linearise, user);
    if (progress_cb)
        progress_cb(1, cfg->max_iterations);
    return fill_outputs(cfg, out, 0);
}

void fabber_nlls_defaults(fvb_nlls *nl)
{
    engine_record("fabber_nlls_defaults");
    nl->lm = 0;
    nl->max_iterations = 200;
    nl->cf_tolerance = 1e-8;
    nl->lambda0 = 0.1;
    nl->lambda_max = 1e20;
}
static void put_nlls(const fvb_nlls *nl)
{
    printf("  nlls lm=%d max_iterations=%d cf_tolerance=%.17g lambda0=%.17g lambda_max=%.17g\n", nl->lm, nl->max_iterations, nl->cf_tolerance,
        nl->lambda0, nl->lambda_max);
}
int32_t fabber_nlls_run_host(const fvb_config *cfg, const fvb_nlls *nl, const void *data, const fvb_outputs *out, int32_t device)
{
    engine_record("fabber_nlls_run_host device=%d", device);
    put_config(cfg);
    put_nlls(nl);
    put_series(cfg, data);
    return fill_outputs(cfg, out, 0);
}
int32_t fabber_nlls_run_hostmodel_host(const fvb_config *cfg, const fvb_nlls *nl, const void *data, const fvb_outputs *out, int32_t device,
    fvb_linearise_fn linearise, void *user)
{
    engine_record("fabber_nlls_run_hostmodel_host device=%d", device);
    put_config(cfg);
    put_nlls(nl);
    put_series(cfg, data);
    call_linearise(cfg, linearise, user);
    return fill_outputs(cfg, out, 0);
}

// (every pointer of cfg is read again here, long after DoCalculations has returned)
int32_t fabber_vb_postproc_host(const fvb_config *cfg, const void *data, const double *mvn, const fvb_postproc *pp, int32_t device)
{
    engine_record("fabber_vb_postproc_host device=%d", device);
    put_config(cfg);
    put_series(cfg, data);
    const int V = cfg->n_voxels, n = cfg->n_params + noise_entries(cfg);
    printf("  mvn last row first=%.17g last=%.17g; postproc set:%s%s%s%s%s%s%s%s -> 0\n", mvn[(size_t)(mvn_rows(n) - 1) * V],
        mvn[(size_t)mvn_rows(n) * V - 1], pp->mean ? " mean" : "", pp->var ? " var" : "", pp->std ? " std" : "", pp->zstat ? " zstat" : "",
        pp->modelfit ? " modelfit" : "", pp->residuals ? " residuals" : "", pp->noise_mean ? " noise_mean" : "", pp->noise_std ? " noise_std" : "");
    const size_t PV = (size_t)cfg->n_params * V, TV = (size_t)cfg->n_times * V, NV = (size_t)noise_entries(cfg) * V;
    struct
    {
        double *p;
        size_t n;
    } images[] = { { pp->mean, PV }, { pp->var, PV }, { pp->std, PV }, { pp->zstat, PV }, { pp->modelfit, TV }, { pp->residuals, TV },
        { pp->noise_mean, NV }, { pp->noise_std, NV } };
    for (size_t i = 0; i < sizeof(images) / sizeof(images[0]); i++)
        for (size_t j = 0; images[i].p && j < images[i].n; j++)
            images[i].p[j] = (double)(i + 1);
    return 0;
}
}
