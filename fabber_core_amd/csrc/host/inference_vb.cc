// inference_vb.cc - the "vb" technique: host driver of the MI355X voxelwise VB engine.
//
// Replaces Vb::Initialize / DoCalculations / SaveResults of the reference
// (inference_vb.cc:100-130, 360-576, 966-1051) and InferenceTechnique::SaveResults
// (inference.cc:112-281). Everything per-voxel happens inside fabber_vb_run_host /
// fabber_vb_postproc_host (HIP kernels); this file only resolves options into the engine's
// problem block, turns per-voxel status words back into the reference's error behaviour, and
// stores the result images in the run data. There is no CPU path: without a GPU the engine
// call fails and the failure is reported as a FabberInternalError.
#include "inference_vb.h"
#include "tools.h"

#include "convergence.h"
#include "engine_binding.h"
#include "host_model.h"
#include "priors.h"
#include "version.h"

#include <cstring>
#include <math.h>
#include <algorithm>
#include <memory>

using namespace std;
using NEWMAT::ColumnVector;
using NEWMAT::Matrix;

// ---------------------------------------------------------------------------------------------
// InferenceTechnique base
// ---------------------------------------------------------------------------------------------
std::vector<std::string> InferenceTechnique::GetKnown()
{
    return InferenceTechniqueFactory::GetInstance()->GetNames();
}

InferenceTechnique *InferenceTechnique::NewFromName(const string &name)
{
    InferenceTechnique *inf = InferenceTechniqueFactory::GetInstance()->Create(name);
    if (!inf)
        throw InvalidOptionValue("method", name, "Unrecognized inference method");
    return inf;
}

void InferenceTechnique::UsageFromName(const string &name, std::ostream &stream)
{
    std::unique_ptr<InferenceTechnique> inf(NewFromName(name));
    stream << "Usage information for method: " << name << endl << endl << inf->GetDescription() << endl << endl << "Options: " << endl << endl;
    vector<OptionSpec> options;
    inf->GetOptions(options);
    for (size_t i = 0; i < options.size(); i++)
        stream << options[i];
}

InferenceTechnique::InferenceTechnique()
    : m_model(NULL)
    , m_num_params(0)
    , m_halt_bad_voxel(true)
{
}

InferenceTechnique::~InferenceTechnique()
{
    for (size_t i = 0; i < resultMVNs.size(); i++)
        delete resultMVNs[i];
}

void InferenceTechnique::Initialize(FwdModel *fwd_model, FabberRunData &rundata)
{
    m_log = rundata.GetLogger();
    m_debug = rundata.GetBool("debug");
    m_model = fwd_model;
    vector<Parameter> params;
    m_model->GetParameters(rundata, params);
    m_num_params = (int)params.size();
    LOG << "InferenceTechnique::Model has " << m_num_params << " parameters" << endl;
    m_masked_tpoints = rundata.GetIntList("mt", 1);
    m_halt_bad_voxel = !rundata.GetBool("allow-bad-voxels");
    LOG << (m_halt_bad_voxel ? "InferenceTechnique::Note: numerical errors in voxels will cause the program to halt.\n"
                               "InferenceTechnique::Use --allow-bad-voxels (with caution!) to keep on calculating.\n"
                             : "InferenceTechnique::Using --allow-bad-voxels: numerical errors in a voxel only stop that voxel.\n");
}

void InferenceTechnique::SaveResults(FabberRunData &rundata) const
{
    if (rundata.GetBool("save-mvn"))
    {
        Matrix image;
        image.ReSizeNoInit(m_result_image.Nrows(), m_result_image.Ncols());
        const size_t cols = (size_t)m_result_image.Ncols();
        const double *src = m_result_image.Store();
        double *dst = image.Store();
        fabber_parallel_for(m_result_image.Nrows(), [=](int r) { memcpy(dst + (size_t)r * cols, src + (size_t)r * cols, sizeof(double) * cols); });
        rundata.SaveVoxelDataMove("finalMVN", image, VDT_MVN);
    }
}

// ---------------------------------------------------------------------------------------------
// Vb
// ---------------------------------------------------------------------------------------------
struct Vb::EngineStorage : EngineBinding { struct Run; };

static OptionSpec VB_OPTIONS[] = {
    { "noise", OPT_STR, "Noise model to use (white or ar1)", OPT_REQ, "" },
    { "host-model-threads", OPT_INT, "Host threads evaluating a host-side model (0 = as many as the hardware has, at most 16)", OPT_NONREQ, "0" },
    { "host-model", OPT_BOOL, "Evaluate the forward model on the host even if it has a device body (always the case for models from a model library)", OPT_NONREQ, "" },
    { "convergence", OPT_STR, "Name of method for detecting convergence", OPT_NONREQ, "maxits" },
    { "max-iterations", OPT_STR, "number of iterations of VB to use with the maxits convergence detector", OPT_NONREQ, "10" },
    { "min-fchange", OPT_STR, "When using the fchange convergence detector, the change in F to stop at", OPT_NONREQ, "10" },
    { "max-trials", OPT_STR, "When using the trial mode convergence detector, the maximum number of trials after an initial reduction in F", OPT_NONREQ, "10" },
    { "print-free-energy", OPT_BOOL, "Output the free energy in the log", OPT_NONREQ, "" },
    { "save-free-energy-history", OPT_BOOL, "Save the free energy of every iteration", OPT_NONREQ, "" },
    { "mcsteps", OPT_INT, "Number of motion correction steps", OPT_NONREQ, "0" },
    { "continue-from-mvn", OPT_MVN, "Continue previous run from output MVN files", OPT_NONREQ, "" },
    { "output-only", OPT_BOOL, "Skip model fitting, just output requested data based on supplied MVN", OPT_NONREQ, "" },
    { "noise-initial-prior", OPT_MATRIX, "MVN of initial noise prior", OPT_NONREQ, "" },
    { "noise-initial-posterior", OPT_MATRIX, "MVN of initial noise posterior", OPT_NONREQ, "" },
    { "noise-pattern", OPT_STR, "repeating pattern of noise variances for each point (e.g. 12 gives odd and even data points different variances)", OPT_NONREQ, "1" },
    { "PSP_byname<n>", OPT_STR, "Name of model parameter to use prior", OPT_NONREQ, "" },
    { "PSP_byname<n>_type", OPT_STR, "Type of prior to use for parameter <n> - I=image prior", OPT_NONREQ, "" },
    { "PSP_byname<n>_image", OPT_IMAGE, "Image prior for parameter <n>", OPT_NONREQ, "" },
    { "PSP_byname<n>_prec", OPT_FLOAT, "Precision to apply to image prior for parameter <n>", OPT_NONREQ, "" },
    { "PSP_byname<n>_transform", OPT_STR, "Transform to apply to parameter <n>", OPT_NONREQ, "" },
    { "allow-bad-voxels", OPT_BOOL, "Continue if numerical error found in a voxel, rather than stopping", OPT_NONREQ, "" },
    { "ar1-cross-terms", OPT_STR, "For AR1 noise, type of cross-linking (dual, same or none)", OPT_NONREQ, "dual" },
    { "num-echoes", OPT_INT, "For AR1 noise, number of interleaved echoes (1 or 2)", OPT_NONREQ, "1" },
    { "spatial-dims", OPT_INT, "Number of spatial dimensions", OPT_NONREQ, "3" },
    { "spatial-speed", OPT_STR, "Restrict speed of spatial smoothing", OPT_NONREQ, "-1" },
    { "param-spatial-priors", OPT_STR, "Type of spatial priors for each parameter, as a sequence of characters. N=nonspatial, M=Markov random field, P=Penny, A=ARD", OPT_NONREQ, "N+" },
    { "locked-linear-from-mvn", OPT_MVN, "MVN file containing fixed centres for linearization", OPT_NONREQ, "" },
    { "spatial-slabs", OPT_BOOL, "With devices=: cut a spatial VB volume into z-slabs over the listed devices (exact, slower than one device; for volumes beyond one device's memory)", OPT_NONREQ, "" },
    { "" },
};

InferenceTechnique *Vb::NewInstance()
{
    return new Vb();
}

Vb::Vb()
    : m_noise(NULL)
    , m_noise_params(0)
    , m_saveF(false)
    , m_saveFsHistory(false)
    , m_printF(false)
    , m_needF(false)
    , m_locked_linear(false)
    , m_nvoxels(0)
    , m_store(new EngineStorage())
{
}

Vb::~Vb()
{
    delete m_noise;
    delete m_store;
}

void Vb::GetOptions(vector<OptionSpec> &opts) const
{
    for (int i = 0; VB_OPTIONS[i].name != ""; i++)
        opts.push_back(VB_OPTIONS[i]);
}

string Vb::GetDescription() const
{
    return "Variational Bayes inference technique (voxelwise), running on the MI355X engine. See Chappell et al IEEE "
           "Trans Sig Proc 57:1 (2009)";
}
string Vb::GetVersion() const
{
    return fabber_version();
}

void Vb::Initialize(FwdModel *fwd_model, FabberRunData &rundata)
{
    InferenceTechnique::Initialize(fwd_model, rundata);
    m_noise = NoiseModel::NewFromName(rundata.GetString("noise"));
    m_noise->Initialize(rundata);
    m_noise_params = m_noise->NumOutputParams();
    LOG << "Vb::Noise has " << m_noise_params << " parameters" << endl;
    m_saveF = rundata.GetBool("save-free-energy");
    m_saveFsHistory = rundata.GetBool("save-free-energy-history");
    m_printF = rundata.GetBool("print-free-energy");
    rundata.GetStringDefault("mcsteps", "0"); // read but unused, as in the reference
    m_locked_linear = rundata.GetStringDefault("locked-linear-from-mvn", "") != "";
}

bool Vb::IsSpatial(FabberRunData &rundata) const
{
    if (rundata.GetString("method") == "spatialvb")
        return true;
    for (size_t k = 0; k < m_store->params.size(); k++)
    {
        switch (m_store->params[k].prior_type)
        {
        case PRIOR_SPATIAL_M:
        case PRIOR_SPATIAL_m:
        case PRIOR_SPATIAL_P:
        case PRIOR_SPATIAL_p:
            return true;
        }
    }
    return false;
}

// a body the model's library supplies counts when the library has registered it with the engine
static bool engine_lists_body(const fvb_config &, const string &body)
{
    bool registered = false;
    for (int i = 0; i < fabber_vb_device_model_count() && !registered; i++)
    {
        const char *name = fabber_vb_device_model_name(i);
        registered = name && body == name;
    }
    return registered;
}

// noise-initial-prior / noise-initial-posterior: ONE distribution from a matrix file for every voxel
// (Vb::InitializeNoiseFromParam, inference_vb.cc:132-142 -> NoiseParams::InputFromMVN); for white noise that is
// a Gamma per precision from its mean and variance (noisemodel_white.cc:70-79, dist_gamma.cc:29-33)
static void noise_distributions_from_files(FabberRunData &rundata, fvb_config &cfg, EasyLog *m_log)
{
    for (const char *key : { "noise-initial-prior", "noise-initial-posterior" })
    {
        const string filename = rundata.GetStringDefault(key, "modeldefault");
        if (filename == "modeldefault")
            continue;
        LOG << "VbInferenceTechnique::Loading " << key << " distribution from " << filename << endl;
        MVNDist dist(filename, m_log);
        // AR(1): the alphas first, then the precisions (Ar1cParams::InputFromMVN, noisemodel_ar.cc:302-316)
        const int nAlpha = (cfg.noise == FVB_NOISE_AR1) ? 2 + cfg.ar_cross_terms : 0;
        if (dist.GetSize() != nAlpha + cfg.n_phis)
            throw InvalidOptionValue(key, filename, "The distribution has " + stringify(dist.GetSize()) + " entries, the noise model "
                    + stringify(nAlpha + cfg.n_phis));
        const NEWMAT::SymmetricMatrix &cov = dist.GetCovariance();
        const bool prior = string(key) == "noise-initial-prior";
        if (nAlpha)
        {
            // alpha.CopyFromSubmatrix(mvn, 1, nAlpha, true): the block must be independent of the rest (dist_mvn.cc:157-165)
            for (int i = 1; i <= nAlpha; i++)
                for (int j = nAlpha + 1; j <= nAlpha + cfg.n_phis; j++)
                    if (cov(i, j) != 0)
                        throw FabberRunDataError("Covariance found in part of MVN that should be independent from the rest!");
            NEWMAT::SymmetricMatrix block(cov.SymSubMatrix(1, nAlpha));
            // a distribution over the alphas has a positive definite covariance (the reference would carry its inverse
            // - whatever it is - into UpdateAlpha and the free energy)
            NEWMAT::SymmetricMatrix inverse;
            bool usable = true;
            try
            {
                inverse = block.i();
            }
            catch (...)
            {
                usable = false;
            }
            for (int i = 1; usable && i <= nAlpha; i++)
                usable = block(i, i) > 0 && inverse(i, i) > 0 && inverse(i, i) - inverse(i, i) == 0;
            if (!usable)
                throw InvalidOptionValue(key, filename, "The covariance of the AR(1) coefficients needs to be positive definite");
            cfg.ar_alpha_given |= prior ? 1 : 2;
            for (int i = 0; i < nAlpha; i++)
            {
                (prior ? cfg.ar_alpha_prior_mean : cfg.ar_alpha_post_mean)[i] = dist.means(i + 1);
                for (int j = 0; j < nAlpha; j++)
                {
                    if (prior)
                        cfg.ar_alpha_prior_prec[i][j] = inverse(i + 1, j + 1); // MVNDist::GetPrecisions
                    else
                        cfg.ar_alpha_post_cov[i][j] = block(i + 1, j + 1);
                }
            }
        }
        for (int i = nAlpha + 1; i <= nAlpha + cfg.n_phis; i++) // WhiteParams::InputFromMVN, noisemodel_white.cc:70-79; noisemodel_ar.cc:311-315
            for (int j = i + 1; j <= nAlpha + cfg.n_phis; j++)
                if (cov(i, j) != 0)
                    throw FabberRunDataError("Phis should have zero covariance!");
        for (int i = 0; i < cfg.n_phis; i++)
        {
            // a Gamma distribution has a positive mean and a positive variance (the reference would carry a
            // negative scale or a division by zero into its first update)
            const int q = nAlpha + i + 1;
            if (!(dist.means(q) > 0) || !(cov(q, q) > 0))
                throw InvalidOptionValue(key, filename, "Noise precision " + stringify(i + 1) + " needs a positive mean and a positive variance");
            const double b = cov(q, q) / dist.means(q); // GammaDist::SetMeanVariance
            const double c = dist.means(q) / b;
            (prior ? cfg.noise_prior_b : cfg.noise_post_b)[i] = b;
            (prior ? cfg.noise_prior_c : cfg.noise_post_c)[i] = c;
        }
    }
}

// The convergence detector. Returns whether the free energy is computed: it or an output reads it (inference_vb.cc:242).
static bool convergence_section(FabberRunData &rundata, fvb_config &cfg, bool outputs_read_f, bool save_history)
{
    std::unique_ptr<ConvergenceDetector> conv(
        ConvergenceDetector::NewFromName(rundata.GetStringDefault("convergence", "maxits")));
    conv->Initialize(rundata);
    cfg.convergence = conv->DeviceCode();
    cfg.max_iterations = conv->MaxIterations();
    cfg.max_trials = conv->MaxTrials();
    cfg.min_fchange = conv->MinFChange();
    const bool need_f = conv->UseF() || outputs_read_f;
    cfg.need_f = need_f ? 1 : 0;
    // every iteration pushes one value and the end of the voxel one more; trial mode and LM can
    // run more iterations than max-iterations
    cfg.f_history_rows = save_history ? (cfg.max_iterations + 2) * (conv->UseF() ? 12 : 1) : 0;
    return need_f;
}

// continue-from-mvn: the given image is the initial posterior (n_noise: the noise model's entries in it)
static void resume_section(FabberRunData &rundata, EngineBinding &st, int n_noise, EasyLog *m_log)
{
    fvb_config &cfg = st.cfg;
    try
    {
        st.init_mvn = rundata.GetVoxelData("continue-from-mvn");
    }
    catch (DataNotFound &)
    {
        return;
    }
    LOG << "Vb::Continuing from MVN" << endl;
    const int rows = fabber_vb_mvn_rows(cfg.n_params + n_noise);
    if (st.init_mvn.Nrows() != rows)
        throw FabberRunDataError("MVNDist::Load  - Incorrect number of rows for an MVN input");
    if (st.init_mvn.Ncols() != cfg.n_voxels)
        throw FabberRunDataError("MVNDist::Load - MVN input has the wrong number of voxels");
    for (int v = 0; v < cfg.n_voxels; v++)
        if (st.init_mvn.at0(rows - 1, v) != 1)
            throw FabberRunDataError("MVNDist::Load - Voxel data does not contain a valid MVN - last value != 1");
    cfg.init_mvn = st.init_mvn.Store();
    rundata.GetStringDefault("continue-from-params", "");
}

// (cfg is the store's own block: everything it points into lives next to it)
void Vb::BuildEngineConfig(FabberRunData &rundata, fvb_config &cfg)
{
    EngineStorage &st = *m_store;
    st.Begin(m_model, rundata);
    // A model without a device body (any model library written for the reference), or any model
    // when host-model is set, is evaluated on the host: 2P+1 Evaluate calls per voxel and
    // re-centre, everything else on the GPU (fabber_vb_run_hostmodel_host).
    st.BindModel(m_model, rundata, &engine_lists_body);
    st.BindParameters(rundata);
    m_noise->ConfigureEngine(cfg, cfg.n_times, st.phi_index);
    cfg.phi_index = st.phi_index.empty() ? NULL : st.phi_index.data();
    noise_distributions_from_files(rundata, cfg, m_log);
    m_needF = convergence_section(rundata, cfg, m_printF || m_saveF || m_saveFsHistory, m_saveFsHistory);
    resume_section(rundata, st, m_noise_params, m_log);
}

// ---- host-evaluated models ----------------------------------------------------------------------

// The initial posterior of every voxel as an MVN image (FwdModel::GetInitialPosterior needs the
// voxel's data, fwdmodel.cc:284-313; noise from the noise model's initial posterior)
void Vb::BuildInitialMvn(FabberRunData &rundata, fvb_config &cfg)
{
    if (cfg.init_mvn)
        return; // continue-from-mvn
    // noise entries of the MVN: white = the precisions; AR(1) = the alphas, then the precisions (noisemodel_ar.cc:287-300)
    const int NA = (cfg.noise == FVB_NOISE_AR1) ? 2 + cfg.ar_cross_terms : 0;
    const int P = cfg.n_params, N = cfg.n_phis, n = P + NA + N, V = cfg.n_voxels;
    const int rows = fabber_vb_mvn_rows(n), nCov = n * (n + 1) / 2;
    const Matrix &data = rundata.GetMainVoxelData();
    const Matrix &coords = rundata.GetVoxelCoords();
    const Matrix &supp = rundata.GetVoxelSuppData();
    Matrix &img = m_store->init_mvn;
    img.ReSize(rows, V);
    img = 0;
    for (int v = 0; v < V; v++)
    {
        if (supp.Ncols() == V)
            m_model->PassData(v + 1, ColumnVector(data.Column(v + 1)), ColumnVector(coords.Column(v + 1)), ColumnVector(supp.Column(v + 1)));
        else
            m_model->PassData(v + 1, ColumnVector(data.Column(v + 1)), ColumnVector(coords.Column(v + 1)));
        MVNDist post(P);
        m_model->GetInitialPosterior(post, rundata);
        const NEWMAT::SymmetricMatrix &cov = post.GetCovariance();
        for (int i = 0; i < P; i++)
        {
            for (int j = 0; j <= i; j++)
                img.at0(i * (i + 1) / 2 + j, v) = cov(i + 1, j + 1);
            img.at0(nCov + i, v) = post.means(i + 1);
        }
        for (int a = 0; a < NA; a++) // Ar1cNoiseModel's initial alpha posterior: N(0, 1e4 I) (noisemodel_ar.cc:379-403),
        {                            // or the one of noise-initial-posterior
            const int q = P + a;
            if (cfg.ar_alpha_given & 2)
            {
                for (int a2 = 0; a2 <= a; a2++)
                    img.at0(q * (q + 1) / 2 + P + a2, v) = cfg.ar_alpha_post_cov[a][a2];
                img.at0(nCov + q, v) = cfg.ar_alpha_post_mean[a];
            }
            else
                img.at0(q * (q + 1) / 2 + q, v) = 1e4;
        }
        for (int k = 0; k < N; k++)
        {
            const double b = cfg.noise_post_b[k], c = cfg.noise_post_c[k];
            const int q = P + NA + k;
            img.at0(q * (q + 1) / 2 + q, v) = b * b * c; // GammaDist variance / mean, as OutputAsMVN
            img.at0(nCov + q, v) = b * c;
        }
        img.at0(rows - 1, v) = 1;
    }
    cfg.init_mvn = img.Store();
}

int32_t Vb::LineariseCallback(void *user, int32_t n_active, const int32_t *ids, const double *means, double *lin)
{
    return host_model_linearise(user, n_active, ids, means, lin);
}

// The engine's per-iteration callback carries no context pointer: the run data whose ProgressCheck should hear
// about spatial iterations (inference_vb.cc:610) is kept per thread, for as long as a spatial run's scope lasts.
static thread_local FabberRunData *s_progress_rundata = NULL;
static void spatial_progress(int it, int maxits)
{
    if (s_progress_rundata)
        s_progress_rundata->Progress(it, maxits);
}
struct SpatialProgressScope
{
    explicit SpatialProgressScope(FabberRunData &rundata) { s_progress_rundata = &rundata; }
    ~SpatialProgressScope() { s_progress_rundata = NULL; }
};

// devices=0,1,...: the list; empty for "" and for "all"
static vector<int32_t> parse_devices(const string &devices_opt)
{
    vector<int32_t> device_list;
    if (devices_opt == "" || devices_opt == "all")
        return device_list;
    for (size_t begin = 0, end; begin <= devices_opt.size(); begin = end + 1)
    {
        end = std::min(devices_opt.find(',', begin), devices_opt.size());
        if (end == begin)
            throw InvalidOptionValue("devices", devices_opt, "Must be 'all' or a comma-separated list of device indices");
        device_list.push_back(convertTo<int>(devices_opt.substr(begin, end - begin)));
    }
    return device_list;
}

// One DoCalculations past its set-up: what the three routes to the engine share. Each route answers the engine's code.
struct Vb::EngineStorage::Run
{
    Vb &vb;
    FabberRunData &rundata;
    FabberStageTimer &timer;
    EngineStorage &st;
    fvb_config &cfg; // (st.cfg)
    EasyLog *m_log;
    fvb_outputs out;
    const void *series;
    // devices=all | devices=0,1,...: voxelwise VB shards the voxel list over several GPUs of the node
    // (fabber_vb_run_host_multi); everything else runs on the first of them (or on device=<index>)
    string devices_opt;
    vector<int32_t> device_list;
    int device;
    vector<double> locked_centres; // [P][V], spatial VB under locked-linear-from-mvn
    HostModelContext host; // (for a model evaluated on the host)
    void LibraryInitialPosterior();
    int Spatial();
    int VoxelwiseHostModel();
    int VoxelwiseDevice();
};

// The initial posterior of a library's device body: where its library compiled the initial-posterior kernel around the
// body's init_posterior (include/fabber_device_init_model.h) the engine writes the image itself, on the device, ahead
// of the fit; else the model's host code does, one voxel after the other (BuildInitialMvn). A lap of its own either
// way, for FVB_HOST_TIMING to tell the two apart.
void Vb::EngineStorage::Run::LibraryInitialPosterior()
{
    if (st.uses_suppdata)
        LOG << "Vb::the body receives " << cfg.n_model_supp << " rows of supplementary data" << endl;
    timer.lap("up to the initial posterior");
    const string kernel = fabber_vb_init_posterior_kernel_name(&cfg);
    if (kernel.empty()) // (continue-from-mvn included: the given image is the initial posterior)
    {
        vb.BuildInitialMvn(rundata, cfg);
        timer.lap("initial posterior on the host (one thread)");
        return;
    }
    LOG << "Vb::the initial posterior comes from the body '" << cfg.device_model << "' of its library (kernel " << kernel << ")" << endl;
    timer.lap("initial posterior left to the engine (kernel on the device)");
}

// Vb::DoCalculationsSpatial (inference_vb.cc:578-767): whole-volume sweeps with the counting
// detector; options as SpatialPrior reads them (priors.cc:190-211)
int Vb::EngineStorage::Run::Spatial()
{
    const int V = cfg.n_voxels;
    const Matrix &coords = *host.coords;
    fvb_spatial sp;
    memset(&sp, 0, sizeof(sp));
    sp.spatial_dims = rundata.GetIntDefault("spatial-dims", 3, 0, 3);
    if (sp.spatial_dims == 1)
        WARN_ONCE("spatial-dims=1 is weird... hope you're just testing!");
    else if (sp.spatial_dims == 2)
        WARN_ONCE("spatial-dims=2 may not work the way you expect");
    sp.spatial_speed = rundata.GetDoubleDefault("spatial-speed", -1);
    sp.update_first_iter = rundata.GetBool("update-spatial-prior-on-first-iteration") ? 1 : 0;
    sp.q1 = rundata.GetDoubleDefault("spatial-q1", 10.0);
    sp.q2 = rundata.GetDoubleDefault("spatial-q2", 1.0);
    if (coords.Nrows() < 3 || coords.Ncols() != V)
        throw FabberInternalError("Vb::CalcNeighbours: voxel co-ordinates do not match the data");
    vector<int32_t> grid((size_t)3 * V);
    for (int d = 0; d < 3; d++)
        for (int v = 0; v < V; v++)
            grid[(size_t)d * V + v] = (int32_t)coords.at0(d, v);
    sp.coords = grid.data();
    sp.locked_centres = locked_centres.empty() ? NULL : locked_centres.data();
    cfg.convergence = FVB_CONV_MAXITS;
    cfg.max_iterations = convertTo<int>(rundata.GetStringDefault("max-iterations", "10"));
    cfg.f_history_rows = 0;
    out.f_history = NULL;
    out.f_history_len = NULL;
    LOG << "Vb::Spatial calculations on the MI355X engine, " << V << " voxels x " << cfg.n_times
        << " timepoints, " << cfg.max_iterations << " iterations" << endl;
    SpatialProgressScope progress(rundata);
    // devices= shards VOXELWISE VB. Spatial VB over several devices (z-slabs, pipelined first sweep) is exact but
    // slower than one device - the ordered sweep is a latency chain that more devices do not shorten - so it
    // is an explicit choice (spatial-slabs) for volumes beyond one device's memory.
    const bool slabs = rundata.GetBool("spatial-slabs");
    if (devices_opt != "" && !slabs)
        WARN_ONCE("devices= shards voxelwise VB only: this spatial VB run uses one device (the faster choice; "
                  "--spatial-slabs cuts the volume into z-slabs over the listed devices for volumes beyond one device's memory)");
    int rc = 0;
    if (st.has_device_model && devices_opt != "" && slabs && !sp.locked_centres)
    {
        // devices=all | devices=0,1,...: z-slabs of the volume on several GPUs, pipelined first sweep
        LOG << "Vb::devices=" << devices_opt << ": the volume is cut into z-slabs" << endl;
        rc = fabber_vb_run_spatial_host_multi(&cfg, &sp, series, &out, device_list.empty() ? NULL : device_list.data(), (int32_t)device_list.size(), spatial_progress);
    }
    else if (st.has_device_model)
    {
        const char *kernels = st.library_device_model ? fabber_vb_spatial_kernel_name(&cfg) : "";
        if (kernels[0])
        {
            // the library brought spatial kernels for this parameter count and noise model; they know no model's
            // InitVoxelPosterior: the initial posterior comes from the library's kernel for it, or from the model's
            // host code
            LOG << "Vb::the model runs on the device with the body '" << cfg.device_model << "' of its library, kernels "
                << kernels << endl;
            LibraryInitialPosterior();
        }
        rc = fabber_vb_run_spatial_host(&cfg, &sp, series, &out, device, spatial_progress);
    }
    if (st.has_device_model && rc == -40)
    {
        // no spatial kernels were built for this model with this many parameters: the model's own host code does the
        // re-centres instead (up to 32 parameters; more than 8 under white noise with one precision). The host route
        // below and SaveResults see the block as rewritten here.
        if (st.uses_suppdata && cfg.n_model_supp > 0)
            LOG << "Vb::the model's library has no spatial entry for this parameter count and noise model, so its body is handed "
                   "no supplementary data under spatial VB: the model runs on the host route" << endl;
        else
            LOG << "Vb::no device kernels for spatial VB with " << cfg.n_params << " parameters of this model" << endl;
        st.has_device_model = st.library_device_model = false;
        cfg.model = FVB_MODEL_HOSTJAC;
        cfg.design = NULL;
        cfg.model_supp = NULL;
        cfg.n_model_supp = 0;
    }
    if (!st.has_device_model)
    {
        // any FwdModel under spatial VB, as in the reference: the model's two re-centres per iteration
        // run here on the host, the sweeps on the device (fabber_vb_run_spatial_hostmodel_host)
        LOG << "Vb::the model is evaluated on the host" << endl;
        vb.BuildInitialMvn(rundata, cfg);
        const int nthreads = host_model_instances(host, cfg, series, m_log); // (its own log lines first)
        LOG << "Vb::Model evaluations on " << nthreads << " host thread(s)" << endl;
        rc = fabber_vb_run_spatial_hostmodel_host(&cfg, &sp, series, &out, device, &Vb::LineariseCallback, &host, spatial_progress);
        host_model_rethrow(host, rc);
    }
    return rc;
}

int Vb::EngineStorage::Run::VoxelwiseHostModel()
{
    LOG << "Vb::Voxelwise calculations on the MI355X engine with the model evaluated on the host, " << cfg.n_voxels
        << " voxels x " << cfg.n_times << " timepoints" << endl;
    vb.BuildInitialMvn(rundata, cfg);
    const int nthreads = host_model_instances(host, cfg, series, m_log); // (its own log lines first)
    LOG << "Vb::Model evaluations on " << nthreads << " host thread(s)" << endl;
    const int rc = fabber_vb_run_hostmodel_host(&cfg, series, &out, device, &Vb::LineariseCallback, &host);
    host_model_rethrow(host, rc);
    return rc;
}

int Vb::EngineStorage::Run::VoxelwiseDevice()
{
    if (st.library_device_model)
    {
        // the fit kernels know no model's InitVoxelPosterior: the initial posterior comes from the library's kernel for
        // it, or from the model's host code
        LOG << "Vb::the model runs on the device with the body '" << cfg.device_model << "' of its library" << endl;
        LibraryInitialPosterior();
    }
    LOG << "Vb::Voxelwise calculations on the MI355X engine, kernel " << fabber_vb_kernel_name(&cfg) << ", "
        << cfg.n_voxels << " voxels x " << cfg.n_times << " timepoints" << endl;
    if (devices_opt == "")
        return fabber_vb_run_host(&cfg, series, &out, device);
    fvb_summary total;
    const int rc = fabber_vb_run_host_multi(&cfg, series, &out, device_list.empty() ? NULL : device_list.data(), (int32_t)device_list.size(), &total);
    if (rc == 0)
        LOG << "Vb::devices=" << devices_opt << ": " << total.sum_iterations << " voxel-iterations, " << total.bad_voxels
            << " voxels stopped on a numerical error" << (vb.m_needF ? ", global free energy " : "")
            << (vb.m_needF ? stringify(total.sum_free_energy) : string("")) << endl;
    return rc;
}

// inference_vb.cc:171-181,225-232: the means of the first P entries of the given MVN image ("does not check
// if the correct number of parameters is present"); MVNDist::Load's checks (dist_mvn.cc:324-374)
static vector<double> load_locked_centres(FabberRunData &rundata, int P, int V, EasyLog *m_log)
{
    const string file = rundata.GetString("locked-linear-from-mvn");
    LOG << "Vb::Loading fixed linearization centres from the MVN '" << file << "'" << endl;
    const Matrix &mvn = rundata.GetVoxelData(file);
    if (mvn.Ncols() == 0)
        throw FabberRunDataError("MVNDist::Load - Voxel data is empty");
    const int n = ((int)sqrt(double(8 * mvn.Nrows() + 1)) - 3) / 2;
    if (mvn.Nrows() != n * (n + 1) / 2 + n + 1)
        throw FabberRunDataError("MVNDist::Load  - Incorrect number of rows for an MVN input");
    if (n < P || mvn.Ncols() != V)
        throw FabberRunDataError("locked-linear-from-mvn: the MVN does not hold the model's parameters for every voxel");
    const int nCov = n * (n + 1) / 2;
    vector<double> centres((size_t)P * V); // [P][V]
    for (int v = 0; v < V; v++)
    {
        if (mvn.at0(nCov + n, v) != 1)
            throw FabberRunDataError("MVNDist::Load - Voxel data does not contain a valid MVN - last value != 1");
        for (int k = 0; k < P; k++)
            centres[(size_t)k * V + v] = mvn.at0(nCov + k, v);
    }
    return centres;
}

void Vb::DoCalculations(FabberRunData &rundata)
{
    FabberStageTimer timer("Vb::DoCalculations");
    fvb_config &cfg = m_store->cfg;
    BuildEngineConfig(rundata, cfg);
    timer.lap("engine configuration");
    m_nvoxels = cfg.n_voxels;
    m_result_image.ReSizeNoInit(fabber_vb_mvn_rows(cfg.n_params + m_noise_params), m_nvoxels); // (the engine writes every voxel's column)
    m_free_energy.clear();
    m_status.assign(m_nvoxels, 0);
    timer.lap("result image");
    const bool output_only = rundata.GetBool("output-only");
    const bool spatial = IsSpatial(rundata);
    if (m_nvoxels == 0)
        return;
    if (output_only)
    {
        LOG << "Vb::DoCalculations output-only set - not performing any calculations" << endl;
        if (!cfg.init_mvn)
            throw FabberRunDataError("output-only needs continue-from-mvn");
        m_result_image = m_store->init_mvn;
        m_needF = false;
        return;
    }

    EngineStorage::Run run = { *this, rundata, timer, *m_store, cfg, m_log, fvb_outputs(), NULL, "", {}, 0, {},
        { m_model, &rundata, NULL, &rundata.GetVoxelCoords(), &rundata.GetVoxelSuppData(), cfg.n_times, cfg.n_params, "", {}, {} } };
    // (a model evaluated on the host takes its data as NEWMAT columns: the matrix then, for the engine too)
    int series_rows = 0, series_cols = 0;
    run.series = engine_series(rundata, !m_store->has_device_model, cfg.data_f64, series_rows, series_cols);
    // (per-voxel arrays the engine writes in full are sized without being filled, and come from the block cache; the free
    // energy - 9999 where the reference stores none, inference_vb.cc:165 - is asked for only when somebody reads it)
    std::vector<int, NEWMAT::DefaultInitAllocator<int> > iterations((size_t)m_nvoxels);
    vector<int> hist_len;
    if (m_needF)
        m_free_energy.assign(m_nvoxels, 9999);
    run.out = { m_result_image.Store(), m_needF ? m_free_energy.data() : NULL, NULL, NULL, m_status.data(), iterations.data() };
    if (cfg.f_history_rows > 0)
    {
        m_f_history.ReSize(cfg.f_history_rows, m_nvoxels);
        hist_len.assign(m_nvoxels, 0);
        run.out.f_history = m_f_history.Store();
        run.out.f_history_len = hist_len.data();
    }
    run.devices_opt = rundata.GetStringDefault("devices", "");
    run.device_list = parse_devices(run.devices_opt);
    run.device = run.device_list.empty() ? rundata.GetIntDefault("device", 0, 0) : run.device_list[0];
    // In the voxelwise loop the locked centres only serve the set-up re-centre, which the loop
    // repeats about the posterior means before anything uses it (inference_vb.cc:227-235, :443,
    // :490): no effect on the results. The spatial loop really keeps them (:695).
    if (m_locked_linear && !spatial)
        LOG << "Vb::locked-linear-from-mvn has no effect on voxelwise VB (the loop re-centres about the posterior means)" << endl;
    if (m_locked_linear && spatial)
        run.locked_centres = load_locked_centres(rundata, cfg.n_params, m_nvoxels, m_log);

    const int rc = spatial ? run.Spatial() : (m_store->has_device_model ? run.VoxelwiseDevice() : run.VoxelwiseHostModel());
    if (rc != 0)
        throw FabberInternalError(string("MI355X engine failed: ") + fabber_vb_last_error());
    timer.lap("engine");

    // ---- per-voxel failures: what the reference's catch blocks do (inference_vb.cc:529-544); the initial ReCentre
    // sits outside the reference's try block (inference_vb.cc:235) ----
    static const char *reasons[] = { "", "LinearizedFwdModel::ReCentre: Non-finite values found in offset",
        "LinearizedFwdModel::ReCentre: Non-finite values found in jacobian", "WhiteNoiseModel::Non-finite free energy!",
        "NEWMAT exception: matrix is singular", "Ar1cNoiseModel: negative variance" };
    static const char *const words[4] = { "Vb::Internal error for voxel ", " : ", "Vb::", " voxels had numerical errors and were stopped early" };
    engine_status_pass(m_status, *run.host.coords, m_halt_bad_voxel, true, reasons, 6, words, m_log);

    if (m_saveFsHistory)
    {
        // pad each voxel's history with its last value up to the longest (inference_vb.cc:1016-1046)
        int longest = 0;
        for (int v = 0; v < m_nvoxels; v++)
            longest = std::max(longest, std::min(hist_len[v], cfg.f_history_rows));
        Matrix hist(longest, m_nvoxels);
        for (int v = 0; v < m_nvoxels; v++)
        {
            const int n = std::min(hist_len[v], cfg.f_history_rows);
            for (int r = 0; r < longest; r++)
                hist.at0(r, v) = m_f_history.at0(r < n ? r : n - 1, v);
        }
        m_f_history = hist;
    }
    timer.lap("status pass");
}

static void save_rows(FabberRunData &rundata, const string &name, const std::vector<double, NEWMAT::DefaultInitAllocator<double> > &buf,
    int rows, int row0, int n_rows, int V)
{
    Matrix m;
    m.ReSizeNoInit(n_rows, V);
    (void)rows;
    if (n_rows > 0 && V > 0)
        memcpy(m.Store(), buf.data() + (size_t)row0 * V, sizeof(double) * (size_t)n_rows * V);
    rundata.SaveVoxelDataMove(name, m);
}

// InferenceTechnique::SaveResults of the reference (inference.cc:112-281) plus the noise images
// of Vb::SaveResults (inference_vb.cc:981-994), from the packed result image by the engine's
// post-processing kernel. N = noise entries in the MVN (0 for NLLS), n_noise_saved = how many of
// them go into noise_means / noise_stdevs.
void InferenceTechnique::SaveEngineResults(FabberRunData &rundata, const fvb_config &cfg, const vector<Parameter> &params,
    int N, int n_noise_saved, bool host_model) const
{
    FabberStageTimer timer("SaveEngineResults");
    InferenceTechnique::SaveResults(rundata); // finalMVN
    timer.lap("finalMVN");

    const int V = cfg.n_voxels, P = cfg.n_params, T = cfg.n_times;
    const bool want_mean = rundata.GetBool("save-mean"), want_std = rundata.GetBool("save-std");
    const bool want_zstat = rundata.GetBool("save-zstat"), want_var = rundata.GetBool("save-var");
    const bool want_nmean = rundata.GetBool("save-noise-mean"), want_nstd = rundata.GetBool("save-noise-std");
    const bool want_fit = rundata.GetBool("save-model-fit"), want_resid = rundata.GetBool("save-residuals");

    // (sized without being written: the post-processing fills them)
    typedef std::vector<double, NEWMAT::DefaultInitAllocator<double> > Image;
    Image mean, var, sd, zstat, fit, resid, nmean, nstd;
    fvb_postproc pp;
    memset(&pp, 0, sizeof(pp));
    const size_t PV = (size_t)P * V, TV = (size_t)T * V, NV = (size_t)N * V;
    if (want_mean)
        mean.resize(PV), pp.mean = mean.data();
    if (want_var)
        var.resize(PV), pp.var = var.data();
    if (want_std)
        sd.resize(PV), pp.std = sd.data();
    if (want_zstat)
        zstat.resize(PV), pp.zstat = zstat.data();
    if (want_fit)
        fit.resize(TV), pp.modelfit = fit.data();
    if (want_resid)
        resid.resize(TV), pp.residuals = resid.data();
    if (want_nmean && N > 0)
        nmean.resize(NV), pp.noise_mean = nmean.data();
    if (want_nstd && N > 0)
        nstd.resize(NV), pp.noise_std = nstd.data();

    if (V > 0)
    {
        fvb_config pcfg = cfg;
        // host_model says which route the FIT took. The prediction depends on the posterior means only: a model of a
        // library takes it from its device body wherever the library compiled the result-image kernel around it
        // (include/fabber_device_results_model.h) - also after a fit on the host route (a library without spatial
        // kernels or minimisers) - unless host-model asks for the host code.
        std::vector<double> constants;
        bool device_fit = false;
        if (host_model && (want_fit || want_resid) && !rundata.GetBool("host-model"))
        {
            DeviceModelSpec spec;
            if (m_model->GetDeviceModel(spec) && !spec.device_model.empty() && spec.device_model.size() < sizeof(pcfg.device_model))
            {
                fvb_config named = cfg;
                named.model = FVB_MODEL_PLUGIN;
                named.design = NULL;
                for (int i = 0; i < 4; i++)
                {
                    named.model_iopt[i] = spec.iopt[i];
                    named.model_dopt[i] = spec.dopt[i];
                }
                memset(named.device_model, 0, sizeof(named.device_model));
                strncpy(named.device_model, spec.device_model.c_str(), sizeof(named.device_model) - 1);
                constants = spec.constants;
                named.model_consts = constants.empty() ? NULL : constants.data();
                named.n_model_consts = (int32_t)constants.size();
                named.model_supp = NULL;
                named.n_model_supp = 0;
                if (spec.uses_suppdata)
                    engine_suppdata(rundata, named);
                const string kernel = fabber_vb_postproc_kernel_name(&named);
                if (kernel.compare(0, 9, "postproc<") == 0)
                {
                    LOG << "InferenceTechnique::model fit and residuals with the body '" << named.device_model
                        << "' of its library (kernel " << kernel << ")" << endl;
                    if (spec.uses_suppdata)
                        LOG << "InferenceTechnique::the body receives " << named.n_model_supp << " rows of supplementary data" << endl;
                    pcfg = named;
                    device_fit = true;
                }
            }
        }
        const bool host_fit = host_model && !device_fit; // the model prediction can only come from the model's own host code
        if (host_fit)
            pp.modelfit = pp.residuals = NULL;
        int series_rows = 0, series_cols = 0;
        // (only the residuals need the series on the device: not uploaded otherwise)
        const void *series = (pp.residuals != NULL) ? engine_series(rundata, host_fit, pcfg.data_f64, series_rows, series_cols) : NULL;
        int rc = fabber_vb_postproc_host(&pcfg, series, m_result_image.Store(), &pp, rundata.GetIntDefault("device", 0, 0));
        if (rc != 0)
            throw FabberInternalError(string("MI355X engine failed in post-processing: ") + fabber_vb_last_error());
        timer.lap("post-processing kernel (host pointers)");
        if (host_fit && (want_fit || want_resid)) // inference.cc:181-243
        {
            const Matrix &data = rundata.GetMainVoxelData();
            const Matrix &coords = rundata.GetVoxelCoords();
            const Matrix &supp = rundata.GetVoxelSuppData();
            const int nCov = (P + N) * (P + N + 1) / 2;
            ColumnVector tmp, means(P);
            for (int v = 0; v < V; v++)
            {
                if (supp.Ncols() == V) // as the voxel loop passes it (inference_vb.cc:104-115)
                    m_model->PassData(v + 1, ColumnVector(data.Column(v + 1)), ColumnVector(coords.Column(v + 1)), ColumnVector(supp.Column(v + 1)));
                else
                    m_model->PassData(v + 1, ColumnVector(data.Column(v + 1)), ColumnVector(coords.Column(v + 1)));
                for (int k = 0; k < P; k++)
                    means(k + 1) = m_result_image.at0(nCov + k, v);
                m_model->EvaluateFabber(means, tmp, "");
                if (tmp.Nrows() != T)
                    throw FabberInternalError("The model's prediction has " + stringify(tmp.Nrows()) + " timepoints, the data " + stringify(T));
                for (int t = 0; t < T; t++)
                {
                    if (want_fit)
                        fit[(size_t)t * V + v] = tmp(t + 1);
                    if (want_resid)
                        resid[(size_t)t * V + v] = data.at0(t, v) - tmp(t + 1);
                }
            }
            timer.lap("model fit and residuals on the host (one thread)");
        }
    }
    for (int k = 0; k < P; k++)
    {
        const string &name = params[k].name;
        if (want_mean)
            save_rows(rundata, "mean_" + name, mean, P, k, 1, V);
        if (want_zstat)
            save_rows(rundata, "zstat_" + name, zstat, P, k, 1, V);
        if (want_std)
            save_rows(rundata, "std_" + name, sd, P, k, 1, V);
        if (want_var)
            save_rows(rundata, "var_" + name, var, P, k, 1, V);
    }
    if (want_resid)
        save_rows(rundata, "residuals", resid, T, 0, T, V);
    if (want_fit)
        save_rows(rundata, "modelfit", fit, T, 0, T, V);
    if (want_nmean && N > 0)
        save_rows(rundata, "noise_means", nmean, N, 0, n_noise_saved, V); // first NumParams() noise entries (inference_vb.cc:981-989)
    if (want_nstd && N > 0)
        save_rows(rundata, "noise_stdevs", nstd, N, 0, n_noise_saved, V);
    timer.lap("images into the run data");

    // model-specific extra outputs are defined by host code only (FwdModel::EvaluateModel with
    // a key): evaluate them on the host, like inference.cc:181-252
    vector<string> outputs;
    m_model->GetOutputs(outputs);
    if (rundata.GetBool("save-model-extras") && !outputs.empty() && V > 0)
    {
        const Matrix &data = rundata.GetMainVoxelData();
        const Matrix &coords = rundata.GetVoxelCoords();
        const int nCov = (P + N) * (P + N + 1) / 2;
        for (size_t o = 0; o < outputs.size(); o++)
        {
            if (outputs[o] == "")
                continue;
            Matrix result;
            ColumnVector tmp, means(P);
            for (int v = 0; v < V; v++)
            {
                try
                {
                    m_model->PassData(v + 1, ColumnVector(data.Column(v + 1)), ColumnVector(coords.Column(v + 1)));
                    for (int k = 0; k < P; k++)
                        means(k + 1) = m_result_image.at0(nCov + k, v);
                    m_model->EvaluateFabber(means, tmp, outputs[o]);
                    if (result.Nrows() != tmp.Nrows())
                        result.ReSize(tmp.Nrows(), V);
                    result.Column(v + 1) = tmp;
                }
                catch (std::exception &e)
                {
                    LOG << "InferenceTechnique::Error generating output " << outputs[o] << " for voxel " << v + 1 << " : " << e.what() << endl;
                }
            }
            rundata.SaveVoxelData(outputs[o], result);
        }
    }

}

void Vb::SaveResults(FabberRunData &rundata) const
{
    LOG << "Vb::Preparing to save results..." << endl;
    SaveEngineResults(rundata, m_store->cfg, m_store->params, m_noise_params, m_noise->NumParams(),
        !m_store->has_device_model || m_store->library_device_model); // (a library's model: SaveEngineResults asks for its result-image kernel)
    const int V = m_nvoxels;
    if (m_saveF && m_needF && !m_free_energy.empty())
    {
        Matrix F(1, V);
        for (int v = 0; v < V; v++)
            F.at0(0, v) = m_free_energy[v];
        rundata.SaveVoxelData("freeEnergy", F);
    }
    else
    {
        LOG << "Vb::Free energy wasn't recorded, so no freeEnergy data saved" << endl;
    }
    if (V > 0 && m_saveFsHistory && m_f_history.Nrows() > 0)
    {
        Matrix hist = m_f_history;
        rundata.SaveVoxelData("freeEnergyHistory", hist);
    }
    LOG << "Vb::Done writing results." << endl;
}
