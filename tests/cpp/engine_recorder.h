// engine_recorder.h - how a test program scripts the recording stand-in for the engine (engine_recorder.cc).
#pragma once

#include <string>
#include <vector>

struct EngineScript
{
    std::vector<std::string> device_models; // the bodies the engine lists (fabber_vb_device_model_name)
    // the kernels the engine names for a library's body ("" = the library brought none)
    std::string init_kernel, spatial_kernel, nlls_kernel, postproc_kernel;
    int rc_spatial_host = 0;   // what fabber_vb_run_spatial_host answers (-40: no spatial kernels for this model)
    std::vector<int> status;   // per voxel, 0 beyond its end
    std::vector<int> hist_len; // per voxel F-history length, f_history_rows beyond its end
};
extern EngineScript engine_script;

/** Starts a scenario: its title line, an empty script, and the next fvb_config record printed in full. */
void engine_begin_scenario(const char *title);

/** One line of the record (printf-style); the driver writes its own lines through it too. */
void engine_record(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
