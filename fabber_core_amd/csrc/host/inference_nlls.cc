// inference_nlls.cc - the "nlls" technique: host driver of the engine's non-linear least squares
// kernel (csrc/vb_nlls_kernel.h). Replaces NLLSInferenceTechnique::Initialize / DoCalculations of
// the reference (inference_nlls.cc:62-214); the per-voxel minimisation, the NLLS precision and
// the result images are computed on the GPU (fabber_nlls_run_host, fabber_vb_postproc_host).
// There is no CPU path.
#include "inference_nlls.h"

#include "engine_binding.h"
#include "host_model.h"
#include "version.h"

#include <cstring>

using namespace std;
using NEWMAT::Matrix;

struct NLLSInferenceTechnique::EngineStorage : EngineBinding {};

static OptionSpec NLLS_OPTIONS[] = {
    { "vb-init", OPT_BOOL, "Whether NLLS is being run in isolation or as a pre-step for VB", OPT_NONREQ, "" },
    { "lm", OPT_BOOL, "Whether to use LM convergence (default is L)", OPT_NONREQ, "" },
    { "host-model-threads", OPT_INT, "Host threads evaluating a host-side model (0 = as many as the hardware has, at most 16)", OPT_NONREQ, "0" },
    { "host-model", OPT_BOOL, "Evaluate the forward model on the host even if it has a device body (always the case for models from a model library without NLLS kernels for a device body)", OPT_NONREQ, "" },
    { "" },
};

InferenceTechnique *NLLSInferenceTechnique::NewInstance()
{
    return new NLLSInferenceTechnique();
}

NLLSInferenceTechnique::NLLSInferenceTechnique()
    : initialFwdPosterior(NULL)
    , m_vbinit(false)
    , m_lm(false)
    , m_store(new EngineStorage())
{
}

NLLSInferenceTechnique::~NLLSInferenceTechnique()
{
    delete initialFwdPosterior;
    delete m_store;
}

void NLLSInferenceTechnique::GetOptions(vector<OptionSpec> &opts) const
{
    for (int i = 0; NLLS_OPTIONS[i].name != ""; i++)
        opts.push_back(NLLS_OPTIONS[i]);
}

string NLLSInferenceTechnique::GetDescription() const
{
    return "Non-linear least squares inference technique, running on the MI355X engine.";
}

string NLLSInferenceTechnique::GetVersion() const
{
    return fabber_version();
}

void NLLSInferenceTechnique::Initialize(FwdModel *fwd_model, FabberRunData &rundata)
{
    InferenceTechnique::Initialize(fwd_model, rundata);
    LOG << "NLLSInferenceTechnique::Initialising" << endl;
    m_vbinit = rundata.GetBool("vb-init");

    // inference_nlls.cc:68-82. NumParams() is the deprecated count the reference uses here; models
    // that describe themselves through GetParameterDefaults only have m_num_params.
    const int n = m_num_params;
    MVNDist *post = new MVNDist(n);
    MVNDist junk(n);
    m_model->HardcodedInitialDists(junk, *post);
    const string file = rundata.GetStringDefault("fwd-inital-posterior", "modeldefault");
    if (file != "modeldefault")
    {
        LOG << "NLLSInferenceTechnique::File posterior" << endl;
        post->LoadFromMatrix(file);
    }
    delete initialFwdPosterior;
    initialFwdPosterior = post;
    if (initialFwdPosterior->GetSize() != n)
        throw FabberInternalError("NLLSInferenceTechnique: starting estimate has " + stringify(initialFwdPosterior->GetSize())
            + " entries, the model has " + stringify(n) + " parameters");
    m_lm = rundata.GetBool("lm");
    LOG << "NLLSInferenceTechnique::Done initialising" << endl;
}

// A body the model's library registered counts when the library also registered NLLS minimisers for it
// (include/fabber_device_nlls_model.h): the engine names a kernel for the configuration then. Without them - a
// library built for voxelwise VB only - and beyond FVB_MAX_PARAMS parameters the model is evaluated on the host.
static bool library_has_minimisers(const fvb_config &named, const string &)
{
    return named.n_params <= FVB_MAX_PARAMS && named.device_model[0] != 0 && fabber_nlls_kernel_name(&named)[0] != 0;
}

void NLLSInferenceTechnique::DoCalculations(FabberRunData &rundata)
{
    EngineStorage &st = *m_store;
    fvb_config &cfg = st.cfg;
    const Matrix &coords = rundata.GetVoxelCoords();
    const void *series = st.Begin(m_model, rundata);
    // the post-processing kernel reads these as for a VB result without noise entries
    cfg.noise = FVB_NOISE_WHITE;
    cfg.n_phis = 0;
    cfg.convergence = FVB_CONV_MAXITS;
    cfg.max_iterations = 1;
    // (a model evaluated on the host: the minimiser's iterations stay on the GPU, fabber_nlls_run_hostmodel_host)
    st.BindModel(m_model, rundata, &library_has_minimisers);
    st.BindParameters(rundata, initialFwdPosterior);
    if (st.Wide() && !st.has_device_model)
        throw FabberInternalError("Models with more than " + stringify(FVB_MAX_PARAMS) + " parameters that are evaluated on the host are not supported under method=nlls by the MI355X engine");
    st.phi_index.clear();
    if (!m_masked_tpoints.empty()) // MaskRows (inference_nlls.cc:110,152,216-234)
    {
        st.phi_index.assign(cfg.n_times, 0);
        for (size_t i = 0; i < m_masked_tpoints.size(); i++)
        {
            const int t = m_masked_tpoints[i];
            if (t < 1 || t > cfg.n_times)
                throw InvalidOptionValue("mt" + stringify(i + 1), stringify(t), "Masked timepoint is outside the time series");
            st.phi_index[t - 1] = 255;
        }
        cfg.phi_index = st.phi_index.data();
    }

    const int V = cfg.n_voxels;
    m_result_image.ReSize(fabber_vb_mvn_rows(cfg.n_params), V);
    m_status.assign(V, 0);
    if (V == 0)
        return;

    fvb_nlls nl;
    fabber_nlls_defaults(&nl);
    nl.lm = m_lm ? 1 : 0; // Levenberg by default, Levenberg-Marquardt with --lm (inference_nlls.cc:124-128)
    vector<int> iterations(V, 0);
    const fvb_outputs out = { m_result_image.Store(), NULL, NULL, NULL, m_status.data(), iterations.data() };
    LOG << "NLLSInferenceTechnique::Calculations on the MI355X engine, " << V << " voxels x " << cfg.n_times << " timepoints, "
        << (m_lm ? "Levenberg-Marquardt" : "Levenberg") << " damping" << endl;
    const int device = rundata.GetIntDefault("device", 0, 0);
    int rc;
    if (st.has_device_model)
    {
        if (st.library_device_model)
            LOG << "NLLSInferenceTechnique::the model runs on the device with the body '" << cfg.device_model << "' of its library, kernel "
                << fabber_nlls_kernel_name(&cfg) << endl;
        if (st.uses_suppdata)
            LOG << "NLLSInferenceTechnique::the body receives " << cfg.n_model_supp << " rows of supplementary data" << endl;
        rc = fabber_nlls_run_host(&cfg, &nl, series, &out, device);
    }
    else
    {
        HostModelContext ctx = { m_model, &rundata, NULL, &coords, &rundata.GetVoxelSuppData(), cfg.n_times, cfg.n_params, "", {}, {} };
        const int nthreads = host_model_instances(ctx, cfg, series, m_log); // (the models read the Matrix form)
        LOG << "NLLSInferenceTechnique::The model is evaluated on the host, " << nthreads << " thread(s)" << endl;
        rc = fabber_nlls_run_hostmodel_host(&cfg, &nl, series, &out, device, &host_model_linearise, &ctx);
        host_model_rethrow(ctx, rc);
    }
    if (rc != 0)
        throw FabberInternalError(string("MI355X engine failed: ") + fabber_vb_last_error());
    rundata.Progress(V, V);

    // per-voxel failures: what the reference's catch block does (inference_nlls.cc:186-207)
    static const char *reasons[] = { "", "LinearizedFwdModel::ReCentre: Non-finite values found in offset",
        "LinearizedFwdModel::ReCentre: Non-finite values found in jacobian", "", "NEWMAT exception: matrix is singular" };
    static const char *const words[4] = { "NLLSInferenceTechnique::NEWMAT Exception in this voxel (", "):\n",
        "NLLSInferenceTechnique::Estimates in ", " voxels may be unreliable (precision matrix set manually)" };
    engine_status_pass(m_status, coords, m_halt_bad_voxel, false, reasons, 5, words, m_log);
}

void NLLSInferenceTechnique::SaveResults(FabberRunData &rundata) const
{
    // (model fit and residuals of a library's model: SaveEngineResults asks for its result-image kernel, as under VB)
    SaveEngineResults(rundata, m_store->cfg, m_store->params, 0, 0, !m_store->has_device_model || m_store->library_device_model);
}
