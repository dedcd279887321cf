// host_model.cc - see host_model.h
#include "host_model.h"

#include "engine_binding.h"

#include <algorithm>
#include <thread>

using namespace std;
using NEWMAT::ColumnVector;

// one model instance per host thread (host-model-threads, default: the hardware's, at most 16): a FwdModel holds the
// current voxel's data, so instances cannot be shared
int host_model_instances(HostModelContext &ctx, fvb_config &cfg, const void *&series, EasyLog *log)
{
    FabberRunData &rundata = *ctx.rundata;
    int nthreads = rundata.GetIntDefault("host-model-threads", 0, 0, 256);
    if (nthreads == 0)
        nthreads = std::max(1, std::min(16, (int)std::thread::hardware_concurrency()));
    ctx.models.push_back(ctx.model);
    for (int k = 1; k < nthreads; k++)
    {
        ctx.copies.emplace_back(FwdModel::NewFromName(rundata.GetString("model")));
        ctx.copies.back()->SetLogger(log);
        ctx.copies.back()->Initialize(rundata);
        vector<Parameter> tmp;
        ctx.copies.back()->GetParameters(rundata, tmp); // resolves the transforms EvaluateFabber applies
        ctx.models.push_back(ctx.copies.back().get());
    }
    ctx.data = &rundata.GetMainVoxelData();
    int rows = 0, cols = 0;
    series = engine_series(rundata, true, cfg.data_f64, rows, cols);
    return nthreads;
}

void host_model_rethrow(const HostModelContext &ctx, int rc)
{
    if (rc == -54 && ctx.error != "")
        throw FabberInternalError(ctx.error);
}

// LinearizedFwdModel::ReCentre (fwdmodel_linear.cc:126-182) for active voxels [a0, a1) with one model instance
static void linearise_range(HostModelContext &cx, FwdModel *model, int a0, int a1, const int32_t *ids, const double *means, double *lin)
{
    const int T = cx.T, P = cx.P;
    const bool have_supp = cx.suppdata->Ncols() == cx.data->Ncols();
    ColumnVector centre(P), pert(P), g, f2, f3;
    for (int a = a0; a < a1; a++)
    {
        const int v = ids[a];
        if (have_supp)
            model->PassData(v + 1, ColumnVector(cx.data->Column(v + 1)), ColumnVector(cx.coords->Column(v + 1)),
                ColumnVector(cx.suppdata->Column(v + 1)));
        else
            model->PassData(v + 1, ColumnVector(cx.data->Column(v + 1)), ColumnVector(cx.coords->Column(v + 1)));
        for (int i = 0; i < P; i++)
            centre(i + 1) = means[(size_t)a * P + i];
        double *out = lin + (size_t)a * T * (P + 1);
        model->EvaluateFabber(centre, g, "");
        if (g.Nrows() != T)
            throw FabberInternalError("Model returned " + stringify(g.Nrows()) + " timepoints, data has " + stringify(T));
        for (int t = 0; t < T; t++)
            out[t] = g(t + 1);
        for (int i = 0; i < P; i++)
        {
            double delta = centre(i + 1) * 1e-5; // :157-161
            if (delta < 0)
                delta = -delta;
            if (delta < 1e-10)
                delta = 1e-10;
            pert = centre;
            pert(i + 1) = centre(i + 1) + delta;
            const double c2 = pert(i + 1);
            model->EvaluateFabber(pert, f2, "");
            pert(i + 1) = centre(i + 1) - delta;
            const double c3 = pert(i + 1);
            model->EvaluateFabber(pert, f3, "");
            for (int t = 0; t < T; t++)
                out[T + (size_t)t * P + i] = (f2(t + 1) - f3(t + 1)) / (c2 - c3);
        }
    }
}

int32_t host_model_linearise(void *user, int32_t n_active, const int32_t *ids, const double *means, double *lin)
{
    HostModelContext &cx = *static_cast<HostModelContext *>(user);
    const int nthreads = std::max(1, std::min((int)cx.models.size(), n_active / 64 + 1));
    std::vector<std::string> errors(nthreads);
    auto work = [&](int k) {
        try
        {
            const int a0 = (int)((long long)n_active * k / nthreads), a1 = (int)((long long)n_active * (k + 1) / nthreads);
            linearise_range(cx, cx.models[k], a0, a1, ids, means, lin);
        }
        catch (std::exception &e)
        {
            errors[k] = e.what();
        }
        catch (...)
        {
            errors[k] = "unknown exception in the model";
        }
    };
    std::vector<std::thread> pool;
    for (int k = 1; k < nthreads; k++)
        pool.emplace_back(work, k);
    work(0);
    for (size_t k = 0; k < pool.size(); k++)
        pool[k].join();
    for (int k = 0; k < nthreads; k++)
        if (errors[k] != "")
        {
            cx.error = errors[k];
            return 1;
        }
    return 0;
}
