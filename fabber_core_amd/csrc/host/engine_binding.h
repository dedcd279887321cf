// engine_binding.h - a forward model and its parameters mapped onto the engine's problem block (fvb_config of
// include/fabber_vb.h), with everything the block points into; written once for the techniques that drive the engine:
// method=vb / spatialvb (inference_vb.cc) and method=nlls (inference_nlls.cc). Internal to the host library.
#pragma once

#include "dist_mvn.h"
#include "fwdmodel.h"
#include "rundata.h"

#include "../../../include/fabber_vb.h"

#include <string>
#include <vector>

/** The main series as the engine reads it: float32 where the run data holds it so (every volume set through the C ABI,
 *  FabberRunData::SetVoxelDataF32), else the double matrix. as_matrix: the caller needs the matrix anyway (a model
 *  evaluated on the host is handed NEWMAT columns). */
const void *engine_series(FabberRunData &rundata, bool as_matrix, int32_t &data_f64, int &rows, int &cols);

/** The run's supplementary data as a library's device body reads it (DeviceModelSpec::uses_suppdata): the matrix is
 *  timepoints x voxels with the voxel fastest, which is the engine's layout, so its store is handed over as it is - the
 *  run data keeps it for the run. Without one value per voxel there is none (NULL, 0 rows): the body's own bound check
 *  then stops every voxel with the non-finite-offset status, as with too few constants. */
void engine_suppdata(FabberRunData &rundata, fvb_config &cfg);

/** cfg and what it points into: it stays where it is, in the technique's store (SaveResults reads cfg long after
 *  DoCalculations). */
struct EngineBinding
{
    fvb_config cfg;
    std::vector<Parameter> params;
    NEWMAT::Matrix design;                          // T x P row-major = engine layout
    std::vector<unsigned char> phi_index;           // per timepoint
    std::vector<std::vector<double> > image_priors; // per parameter
    NEWMAT::Matrix init_mvn;                        // continue-from-mvn, or the model's own initial posteriors
    std::vector<double> constants;                  // of a library's body (fvb_config.model_consts)
    bool has_device_model = false;     // the model runs on the device ...
    bool library_device_model = false; // ... with a body of its own library (FVB_MODEL_PLUGIN)
    bool uses_suppdata = false;        // ... which reads the voxels' supplementary data (fvb_config.model_supp)

    EngineBinding() = default;
    EngineBinding(const EngineBinding &) = delete;
    EngineBinding &operator=(const EngineBinding &) = delete;

    /** A new block of the series' shape (returned: engine_series) with the model's parameters, FVB_MAX_PARAMS_EXT at most. */
    const void *Begin(FwdModel *model, FabberRunData &rundata);
    bool Wide() const { return cfg.n_params > FVB_MAX_PARAMS; }
    /** The model section. A model without a device body, or any model when host-model is set, is evaluated on the host
     *  (FVB_MODEL_HOSTJAC). Whether a body of the model's own library counts is the technique's decision: accept_body sees
     *  the block as it would be with the body (name, constants, supplementary data; not for a name too long) and the name. */
    typedef bool (*AcceptBody)(const fvb_config &named, const std::string &name);
    void BindModel(FwdModel *model, FabberRunData &rundata, AcceptBody accept_body);
    /** The per-parameter section: transforms, priors (image priors from the run data) and initial posteriors; for a
     *  minimiser the transforms and its starting estimate (Fabber space) alone, everything else zero. */
    void BindParameters(FabberRunData &rundata, const MVNDist *minimiser_start = NULL);

private:
    // the per-parameter entries: in cfg itself, or - more than FVB_MAX_PARAMS parameters - as a table (cfg.params_ext)
    struct Slots
    {
        int32_t *transform, *prior_type;
        double *prior_mean, *prior_var, *prior_prec, *post_mean, *post_var;
        const double **image_prior;
    };
    Slots ParameterSlots();
    std::vector<int32_t> wide_ints;    // [2][P]
    std::vector<double> wide_doubles;  // [5][P]
    std::vector<const double *> wide_images;
    fvb_param_table wide;
};

/** The per-voxel failures the engine reports, as the reference's catch blocks word them: logs the first 20 bad voxels and
 *  their number; throws at the first one if halt is set or - halt_in_setup - it failed during set-up (status bit 0x100).
 *  reasons: by status code (beyond n_reasons: as code 4). words: around "<voxel> at <x> <y> <z>", around the number. */
void engine_status_pass(const std::vector<int> &status, const NEWMAT::Matrix &coords, bool halt, bool halt_in_setup,
    const char *const *reasons, int n_reasons, const char *const words[4], EasyLog *log);
