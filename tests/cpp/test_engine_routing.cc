// test_engine_routing.cc - runs the host library's techniques against the recording stand-in for the engine
// (engine_recorder.cc) and prints, scenario by scenario, the stand-in's records, the technique's log lines, the stage-timer
// laps of some runs with the times stripped, and the exception a run ended with. tests/test_engine_routing.py compares the output with
// tests/golden/engine_routing.txt line for line. 6 voxels on a 3x2x1 grid, 10 timepoints.
#include "engine_recorder.h"

#include "../../include/fabber_capi.h"

#define FABBER_TEST_HOST
#define FABBER_TEST_OWN_BODIES // (no device code here: only the models' host classes)
#define FABBER_TEST_MULTIEXP "rec_multiexp"
#define FABBER_TEST_INVREC "rec_invrec"
#define FABBER_TEST_WITH "no kernels"
#include "../plugins/test_device_models.h"

#include "fabber_core/easylog.h"
#include "fabber_core/rundata.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <sstream>
#include <typeinfo>

using NEWMAT::Matrix;
using std::string;

namespace
{
const int NX = 3, NY = 2, V = NX * NY, T = 10;

// inversion recovery whose body reads the voxels' supplementary data
class SuppInvRecFwdModel : public InvRecFwdModel
{
public:
    static FwdModel *NewInstance()
    {
        return new SuppInvRecFwdModel();
    }
    bool GetDeviceModel(DeviceModelSpec &spec) const
    {
        InvRecFwdModel::GetDeviceModel(spec);
        spec.uses_suppdata = true;
        return true;
    }
};

struct RecordingProgress : public ProgressCheck
{
    void Progress(int voxel, int nVoxels)
    {
        engine_record("progress %d of %d", voxel, nVoxels);
    }
};

Matrix grid_coords()
{
    Matrix coords(3, V);
    for (int v = 0; v < V; v++)
    {
        coords(1, v + 1) = v % NX;
        coords(2, v + 1) = v / NX;
        coords(3, v + 1) = 0;
    }
    return coords;
}

double sample(int t, int v)
{
    return 10 + v + 0.5 * t + 0.25 * t * t / (1 << v);
}

Matrix series()
{
    Matrix data(T, V);
    for (int t = 0; t < T; t++)
        for (int v = 0; v < V; v++)
            data(t + 1, v + 1) = sample(t, v);
    return data;
}

// a packed MVN image for n entries: unit covariance, means (k + 1) / 8 + v / 64, last row 1
Matrix mvn_image(int n)
{
    const int nCov = n * (n + 1) / 2;
    Matrix mvn(nCov + n + 1, V);
    mvn = 0;
    for (int v = 0; v < V; v++)
    {
        for (int k = 0; k < n; k++)
        {
            mvn(k * (k + 1) / 2 + k + 1, v + 1) = 1;
            mvn(nCov + k + 1, v + 1) = 0.125 * (k + 1) + v / 64.0;
        }
        mvn(nCov + n + 1, v + 1) = 1;
    }
    return mvn;
}

// [covariance means(:); means(:) 1.0] with a diagonal covariance, as a matrix file
void write_mvn_file(const string &name, const std::vector<double> &means, const std::vector<double> &vars)
{
    std::ofstream out(name.c_str());
    out.precision(17);
    const int n = (int)means.size();
    for (int r = 0; r <= n; r++)
    {
        for (int c = 0; c <= n; c++)
            out << (r == n && c == n ? 1.0 : (r == n ? means[c] : (c == n ? means[r] : (r == c ? vars[r] : 0.0)))) << " ";
        out << "\n";
    }
}

void write_design_file(const string &name, int n_params)
{
    std::ofstream out(name.c_str());
    out.precision(17);
    for (int t = 0; t < T; t++)
    {
        for (int k = 0; k < n_params; k++) // (values with short binary expansions: they print short)
            out << (k == 0 ? 1.0 : ((t * (k + 3)) % 8) / 8.0 + k / 64.0) << " ";
        out << "\n";
    }
}

// log lines left out of the record: what FabberRunData::Run itself writes around the technique (times, its echo of the
// options the scenario set, its stages) - but not which results were saved
bool is_left_out(const string &line)
{
    return line.compare(0, 15, "FabberRunData::") == 0 && line.compare(0, 32, "FabberRunData::Saving to memory:") != 0;
}

// "12.3 ms" -> "# ms"
string without_times(const string &line)
{
    string out;
    for (size_t i = 0; i < line.size();)
    {
        size_t j = i;
        while (j < line.size() && (isdigit((unsigned char)line[j]) || line[j] == '.'))
            j++;
        if (j > i && line.compare(j, 3, " ms") == 0)
        {
            out += "#";
            i = j;
        }
        else
            out += line[i++];
    }
    return out;
}

// the stage-timer laps (names and order) are recorded for the runs between laps(true) and laps(false)
void laps(bool on)
{
    if (on)
        setenv("FVB_HOST_TIMING", "1", 1);
    else
        unsetenv("FVB_HOST_TIMING");
}

void begin(const string &title)
{
    engine_begin_scenario(title.c_str());
    // (fabber_destroy drops the registries: the library's models are entered for every run)
    FwdModelFactory::GetInstance()->Add("rec_multiexp", &MultiExpFwdModel::NewInstance);
    FwdModelFactory::GetInstance()->Add("rec_invrec", &InvRecFwdModel::NewInstance);
    FwdModelFactory::GetInstance()->Add("rec_invrec_supp", &SuppInvRecFwdModel::NewInstance);
    if (!freopen("stage_timer.txt", "w", stderr))
        abort();
}

void end(const string &log)
{
    std::istringstream lines(log);
    string line;
    while (std::getline(lines, line))
        if (!is_left_out(line))
            engine_record("log| %s", line.c_str());
    fflush(stderr);
    std::ifstream laps("stage_timer.txt");
    while (std::getline(laps, line))
        engine_record("stderr| %s", without_times(line).c_str());
}

// a saved image, one line per voxel (a run of equal values as "v xN")
void put_matrix(FabberRunData &rundata, const string &name)
{
    try
    {
        const Matrix &m = rundata.GetVoxelData(name);
        engine_record("saved %s %d x %d, by voxel:", name.c_str(), m.Nrows(), m.Ncols());
        for (int c = 1; c <= m.Ncols(); c++)
        {
            string column;
            for (int r = 1, next; r <= m.Nrows(); r = next)
            {
                for (next = r + 1; next <= m.Nrows() && m(next, c) == m(r, c); next++)
                {
                }
                char text[60];
                snprintf(text, sizeof(text), next - r > 1 ? " %.17g x%d" : " %.17g", m(r, c), next - r);
                column += text;
            }
            engine_record(" %s", column.c_str());
        }
    }
    catch (DataNotFound &)
    {
    }
}

typedef std::vector<std::pair<string, string> > Options;
typedef std::function<void(FabberRunData &)> Setup;

// one run through the class API (the series as a matrix of doubles)
void scenario(const string &title, const Options &options, const Setup &setup = Setup())
{
    begin(title);
    EasyLog log;
    std::stringstream text;
    log.StartLog(text);
    {
        FabberRunData rundata(false); // (none of the save-* options the C ABI sets: the scenario asks for its outputs)
        rundata.SetLogger(&log);
        try
        {
            rundata.SetVoxelCoords(grid_coords());
            rundata.SetVoxelData("data", series());
            for (size_t i = 0; i < options.size(); i++)
                rundata.Set(options[i].first, options[i].second);
            if (setup)
                setup(rundata);
            RecordingProgress progress;
            rundata.Run(&progress);
            log.ReissueWarnings();
            put_matrix(rundata, "freeEnergy");
            put_matrix(rundata, "freeEnergyHistory");
        }
        catch (const std::exception &e)
        {
            log.ReissueWarnings();
            engine_record("threw %s: %s", typeid(e).name(), e.what());
        }
    }
    log.StopLog();
    end(text.str());
}

void capi_progress(int voxel, int n)
{
    engine_record("progress %d of %d", voxel, n);
}

// one run through the C ABI (the series as float32)
void capi_scenario(const string &title, const Options &options)
{
    begin(title);
    char err[FABBER_ERR_MAXC] = "";
    std::vector<char> log(1 << 16, 0);
    void *fab = fabber_new(err);
    std::vector<int> mask(V, 1);
    std::vector<float> data((size_t)T * V);
    for (int t = 0; t < T; t++)
        for (int v = 0; v < V; v++)
            data[(size_t)t * V + v] = (float)sample(t, v);
    int rc = fabber_set_extent(fab, NX, NY, 1, mask.data(), err);
    for (size_t i = 0; rc == 0 && i < options.size(); i++)
        rc = fabber_set_opt(fab, options[i].first.c_str(), options[i].second.c_str(), err);
    if (rc == 0)
        rc = fabber_set_data(fab, "data", T, data.data(), err);
    if (rc == 0)
        rc = fabber_dorun(fab, (unsigned)log.size(), log.data(), err, capi_progress);
    engine_record("C ABI -> %d '%s'", rc, err);
    for (const char *name : { "mean_c0", "modelfit", "freeEnergy", "finalMVN" })
        engine_record("size of %s: %d", name, fabber_get_data_size(fab, name, err));
    fabber_destroy(fab);
    end(log.data());
}

Options operator+(Options a, const Options &b)
{
    a.insert(a.end(), b.begin(), b.end());
    return a;
}
} // namespace

int main()
{
    setvbuf(stdout, NULL, _IONBF, 0);
    write_design_file("design40.mat", 40);
    write_design_file("design3.mat", 3);
    write_mvn_file("ar1_prior.mat", { 0.125, 0.25, 2.0 }, { 4.0, 8.0, 0.5 });
    write_mvn_file("ar1_post.mat", { 0.375, 0.5, 4.0 }, { 2.0, 0.5, 2.0 });
    write_mvn_file("ar2_prior.mat", { 0.125, 0.25, 0.375, 0.5, 2.0, 4.0 }, { 4.0, 8.0, 2.0, 16.0, 0.5, 0.25 });
    write_mvn_file("ar2_post.mat", { 0.5, 0.625, 0.75, 0.875, 4.0, 2.0 }, { 2.0, 0.5, 4.0, 0.25, 2.0, 0.5 });
    write_mvn_file("white2_prior.mat", { 2.0, 4.0 }, { 0.5, 0.25 });
    write_mvn_file("bad_prior.mat", { 2.0 }, { 0.5 });

    const Options poly = { { "model", "poly" }, { "degree", "1" }, { "method", "vb" }, { "noise", "white" }, { "max-iterations", "3" } };
    const Options expo = { { "model", "exp" }, { "dt", "0.1" }, { "num-exps", "1" }, { "method", "vb" }, { "noise", "ar" } };
    const Options fit = { { "save-model-fit", "" }, { "save-residuals", "" }, { "save-mean", "" }, { "save-noise-mean", "" } };
    const Options host_model = { { "host-model", "" }, { "host-model-threads", "2" } };
    const Options wide = { { "model", "linear" }, { "basis", "design40.mat" } };
    const Options multiexp = { { "model", "rec_multiexp" }, { "dt", "0.1" }, { "num-exps", "1" }, { "noise", "white" }, { "host-model-threads", "2" } };
    Options invrec = { { "noise", "white" }, { "host-model-threads", "2" } };
    for (int t = 0; t < T; t++)
        invrec.push_back({ "ti" + stringify(t + 1), stringify(0.25 * (t + 1)) });
    const Setup suppdata = [](FabberRunData &rundata) {
        Matrix supp(2, V);
        for (int v = 0; v < V; v++)
        {
            supp(1, v + 1) = 1 + 0.5 * v;
            supp(2, v + 1) = -v;
        }
        rundata.SetVoxelData("suppdata", supp);
    };

    // ---- voxelwise VB: engine call and configuration ----
    capi_scenario("vb poly white through the C ABI", poly + fit + Options{ { "an-option-nobody-reads", "1" } });
    laps(true);
    scenario("vb poly white", poly);
    laps(false);
    scenario("vb exp ar one echo, noise distributions from files",
        expo + Options{ { "noise-initial-prior", "ar1_prior.mat" }, { "noise-initial-posterior", "ar1_post.mat" } });
    scenario("vb exp ar two echoes, noise distributions from files",
        expo + Options{ { "num-echoes", "2" }, { "ar1-cross-terms", "dual" }, { "noise-initial-prior", "ar2_prior.mat" }, { "noise-initial-posterior", "ar2_post.mat" } });
    scenario("vb exp ar, a distribution of the wrong size", expo + Options{ { "noise-initial-prior", "bad_prior.mat" } });
    scenario("vb poly noise pattern, masked timepoints",
        poly + Options{ { "noise-pattern", "12" }, { "mt1", "3" }, { "mt2", "10" }, { "noise-initial-prior", "white2_prior.mat" } });
    scenario("vb poly image prior", poly + Options{ { "PSP_byname1", "c1" }, { "PSP_byname1_type", "I" }, { "PSP_byname1_image", "slope" }, { "PSP_byname1_prec", "4" } },
        [](FabberRunData &rundata) {
            Matrix image(1, V);
            for (int v = 0; v < V; v++)
                image(1, v + 1) = 0.5 + v;
            rundata.SetVoxelData("slope", image);
        });
    scenario("vb poly image prior without its image", poly + Options{ { "PSP_byname1", "c1" }, { "PSP_byname1_type", "I" }, { "PSP_byname1_image", "slope" } });
    scenario("vb poly image prior, image without rows", poly + Options{ { "PSP_byname1", "c1" }, { "PSP_byname1_type", "I" }, { "PSP_byname1_image", "slope" } },
        [](FabberRunData &rundata) { rundata.SetVoxelData("slope", Matrix(0, V)); });
    scenario("vb poly devices=0,1", poly + Options{ { "devices", "0,1" }, { "print-free-energy", "" } });
    scenario("vb poly devices=all", poly + Options{ { "devices", "all" } });
    scenario("vb poly devices with an empty item", poly + Options{ { "devices", "0,,1" } });
    scenario("vb poly device=1", poly + Options{ { "device", "1" } });
    scenario("vb poly devices=1,0 and device=3", poly + Options{ { "devices", "1,0" }, { "device", "3" } });
    laps(true);
    scenario("vb poly host-model", poly + host_model + fit);
    laps(false);
    scenario("vb linear 40 parameters", wide + Options{ { "method", "vb" }, { "noise", "white" } } + fit);
    scenario("vb linear 40 parameters, image prior",
        wide + Options{ { "method", "vb" }, { "noise", "white" }, { "PSP_byname1", "Parameter_35" }, { "PSP_byname1_type", "I" }, { "PSP_byname1_image", "p35" } },
        [](FabberRunData &rundata) {
            Matrix image(1, V);
            for (int v = 0; v < V; v++)
                image(1, v + 1) = 2 - v;
            rundata.SetVoxelData("p35", image);
        });
    scenario("vb linear, design of the wrong length", Options{ { "model", "linear" }, { "basis", "design3.mat" }, { "method", "vb" }, { "noise", "white" } },
        [](FabberRunData &rundata) { rundata.SetVoxelData("data", Matrix(series().Rows(1, T - 1))); });

    // ---- voxelwise VB: start-up, status and history ----
    scenario("vb poly F history under trialmode, unequal lengths",
        poly + Options{ { "save-free-energy-history", "" }, { "convergence", "trialmode" }, { "max-trials", "2" }, { "save-free-energy", "" } },
        [](FabberRunData &) { engine_script.hist_len = { 3, 1, 7, 2, 1000, 4 }; });
    const Setup resume = [](FabberRunData &rundata) { rundata.SetVoxelData("resume", mvn_image(3)); };
    scenario("vb poly continue-from-mvn", poly + Options{ { "continue-from-mvn", "resume" }, { "continue-from-params", "" } }, resume);
    scenario("vb poly continue-from-params alone", poly + Options{ { "continue-from-params", "" } });
    scenario("vb poly continue-from-mvn output-only", poly + Options{ { "continue-from-mvn", "resume" }, { "output-only", "" } } + fit, resume);
    scenario("vb poly output-only alone", poly + Options{ { "output-only", "" } });
    scenario("vb poly continue-from-mvn of the wrong size", poly + Options{ { "continue-from-mvn", "resume" } },
        [](FabberRunData &rundata) { rundata.SetVoxelData("resume", mvn_image(2)); });
    scenario("vb poly continue-from-mvn, last row not 1", poly + Options{ { "continue-from-mvn", "resume" } }, [](FabberRunData &rundata) {
        Matrix mvn = mvn_image(3);
        mvn(mvn.Nrows(), 4) = 0;
        rundata.SetVoxelData("resume", mvn);
    });
    for (int code : { 4, 0x101 })
        for (int allow = 0; allow < 2; allow++)
            scenario("vb poly status " + stringify(code) + (allow ? " with allow-bad-voxels" : ", halting"), poly + (allow ? Options{ { "allow-bad-voxels", "" } } : Options()),
                [code](FabberRunData &) { engine_script.status = { 0, code, 0, 3 }; });

    // ---- spatial VB ----
    const Options spatial = { { "param-spatial-priors", "M+" } };
    const Setup locked = [](FabberRunData &rundata) { rundata.SetVoxelData("centres", mvn_image(3)); };
    scenario("spatial poly prior M, options away from their defaults",
        poly + spatial + Options{ { "spatial-dims", "2" }, { "spatial-speed", "1.5" }, { "spatial-q1", "5" }, { "spatial-q2", "2" },
                             { "update-spatial-prior-on-first-iteration", "" }, { "save-free-energy-history", "" }, { "convergence", "trialmode" } });
    scenario("spatialvb poly by the method's name", Options{ { "model", "poly" }, { "degree", "1" }, { "method", "spatialvb" }, { "noise", "white" } });
    scenario("spatial poly locked-linear-from-mvn", poly + spatial + Options{ { "locked-linear-from-mvn", "centres" } }, locked);
    scenario("spatial poly locked-linear-from-mvn with too few entries", poly + spatial + Options{ { "locked-linear-from-mvn", "centres" } },
        [](FabberRunData &rundata) { rundata.SetVoxelData("centres", mvn_image(1)); });
    scenario("vb poly locked-linear-from-mvn (voxelwise: not loaded)", poly + Options{ { "locked-linear-from-mvn", "centres" } });
    scenario("vb poly spatial options on the voxelwise route", poly + Options{ { "spatial-dims", "2" }, { "spatial-slabs", "" }, { "spatial-q1", "5" } });
    scenario("spatial poly devices=0,1 without spatial-slabs", poly + spatial + Options{ { "devices", "0,1" } });
    scenario("spatial poly devices=0,1 with spatial-slabs", poly + spatial + Options{ { "devices", "0,1" }, { "spatial-slabs", "" } });
    scenario("spatial poly devices=all with spatial-slabs", poly + spatial + Options{ { "devices", "all" }, { "spatial-slabs", "" } });
    scenario("spatial poly devices=1,0 with spatial-slabs and locked centres",
        poly + spatial + Options{ { "devices", "1,0" }, { "spatial-slabs", "" }, { "locked-linear-from-mvn", "centres" } }, locked);
    scenario("spatial linear, the engine answers -40", Options{ { "model", "linear" }, { "basis", "design3.mat" }, { "method", "spatialvb" }, { "noise", "white" }, { "host-model-threads", "2" } } + fit,
        [](FabberRunData &) { engine_script.rc_spatial_host = -40; });
    scenario("spatial poly host-model", poly + spatial + host_model);

    // ---- a library's device body ----
    laps(true);
    const Setup listed = [](FabberRunData &) { engine_script.device_models = { "another", "rec_multiexp", "rec_invrec" }; };
    scenario("vb library body, initial posterior from the host", multiexp + Options{ { "method", "vb" } } + fit, listed);
    scenario("vb library body, initial posterior from its kernel", multiexp + Options{ { "method", "vb" } } + fit, [&](FabberRunData &rundata) {
        listed(rundata);
        engine_script.init_kernel = "init<rec_multiexp>";
        engine_script.postproc_kernel = "postproc<rec_multiexp>";
    });
    scenario("vb library body, continue-from-mvn", multiexp + Options{ { "method", "vb" }, { "continue-from-mvn", "resume" }, { "devices", "0,1" } }, [&](FabberRunData &rundata) {
        listed(rundata);
        engine_script.init_kernel = "init<rec_multiexp>";
        resume(rundata);
    });
    scenario("vb library body the engine does not list", multiexp + Options{ { "method", "vb" } } + fit,
        [](FabberRunData &) { engine_script.device_models = { "another" }; });
    scenario("vb library body with host-model", multiexp + Options{ { "method", "vb" }, { "host-model", "" } }, listed);
    scenario("vb library body with constants", invrec + Options{ { "model", "rec_invrec" }, { "method", "vb" } }, listed);
    scenario("vb library body reading supplementary data", invrec + Options{ { "model", "rec_invrec_supp" }, { "method", "vb" } } + fit, [&](FabberRunData &rundata) {
        listed(rundata);
        suppdata(rundata);
        engine_script.postproc_kernel = "postproc<rec_invrec>";
    });
    scenario("vb library body reading supplementary data, none given", invrec + Options{ { "model", "rec_invrec_supp" }, { "method", "vb" } }, listed);
    scenario("spatial library body with spatial kernels", multiexp + spatial + Options{ { "method", "vb" } }, [&](FabberRunData &rundata) {
        listed(rundata);
        engine_script.spatial_kernel = "spatial<rec_multiexp,2>";
        engine_script.init_kernel = "init<rec_multiexp>";
    });
    scenario("spatial library body with spatial kernels and supplementary data, initial posterior from the host",
        invrec + spatial + Options{ { "model", "rec_invrec_supp" }, { "method", "vb" } }, [&](FabberRunData &rundata) {
            listed(rundata);
            suppdata(rundata);
            engine_script.spatial_kernel = "spatial<rec_invrec,3>";
        });
    scenario("spatial library body without spatial kernels (-40)", multiexp + spatial + Options{ { "method", "vb" } } + fit, [&](FabberRunData &rundata) {
        listed(rundata);
        engine_script.rc_spatial_host = -40;
    });
    scenario("spatial library body with supplementary data, without spatial kernels (-40)",
        invrec + spatial + Options{ { "model", "rec_invrec_supp" }, { "method", "vb" } } + fit, [&](FabberRunData &rundata) {
            listed(rundata);
            suppdata(rundata);
            engine_script.rc_spatial_host = -40;
            engine_script.postproc_kernel = "postproc<rec_invrec>";
        });

    // ---- NLLS ----
    laps(false);
    const Options nlls_poly = { { "model", "poly" }, { "degree", "2" }, { "method", "nlls" } };
    capi_scenario("nlls poly through the C ABI", nlls_poly + fit);
    scenario("nlls poly", nlls_poly);
    scenario("nlls poly lm", nlls_poly + Options{ { "lm", "" }, { "device", "2" } });
    scenario("nlls poly masked timepoints", nlls_poly + Options{ { "mt1", "1" }, { "mt2", "7" } });
    scenario("nlls poly masked timepoint outside the series", nlls_poly + Options{ { "mt1", "11" } });
    scenario("nlls poly host-model", nlls_poly + host_model + fit);
    scenario("nlls linear 40 parameters", wide + Options{ { "method", "nlls" } } + fit);
    scenario("nlls linear 40 parameters host-model (refused)", wide + Options{ { "method", "nlls" } } + host_model);
    scenario("nlls linear, design of the wrong length", Options{ { "model", "linear" }, { "basis", "design3.mat" }, { "method", "nlls" } },
        [](FabberRunData &rundata) { rundata.SetVoxelData("data", Matrix(series().Rows(1, T - 1))); });
    scenario("nlls library body with minimisers", invrec + Options{ { "model", "rec_invrec_supp" }, { "method", "nlls" } } + fit, [&](FabberRunData &rundata) {
        listed(rundata);
        suppdata(rundata);
        engine_script.nlls_kernel = "nlls_wave<rec_invrec>";
    });
    scenario("nlls library body without minimisers", invrec + Options{ { "model", "rec_invrec_supp" }, { "method", "nlls" } } + fit, [&](FabberRunData &rundata) {
        listed(rundata);
        suppdata(rundata);
        engine_script.postproc_kernel = "postproc<rec_invrec>";
    });
    scenario("nlls library body with host-model", multiexp + Options{ { "method", "nlls" }, { "host-model", "" } }, [&](FabberRunData &rundata) {
        listed(rundata);
        engine_script.nlls_kernel = "nlls<rec_multiexp,2>";
    });
    for (int allow = 0; allow < 2; allow++)
        scenario(string("nlls poly bad voxels") + (allow ? " with allow-bad-voxels" : ", halting"), nlls_poly + (allow ? Options{ { "allow-bad-voxels", "" } } : Options()),
            [](FabberRunData &) { engine_script.status = { 0, 2, 0x104, 0, 9 }; });
    engine_record("==== end");
    return 0;
}
