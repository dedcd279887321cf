/*
 * fabber_device_lane_noise_model.h - the lane-per-voxel kernels for a model library's DEVICE body under AR(1) noise and
 * under a noise pattern.
 *
 * fabber_device_lane_model.h gives a body the lane kernels of white noise with one precision. This header compiles the
 * engine's other two lane-kernel families around the SAME body, for one parameter count per macro line:
 *
 *     FABBER_DEVICE_MODEL("invrec", InvRec)          // the wave kernels: the route of everything not covered below
 *     FABBER_DEVICE_LANE_NOISE_MODEL("invrec", InvRec, 3, FVB_LANE_NOISE_AR1 | FVB_LANE_NOISE_PHIS)
 *
 * The first line is required: an entry without a wave body of the same name is never used. A FABBER_DEVICE_LANE_MODEL line
 * is not: the white-noise lane kernels are an entry of their own. Several lines per name are allowed, each for
 * 1 <= P <= 6. It is a header of its own because it includes the kernels of both families: a library that does not want
 * them does not pay for them. Compile as fabber_device_model.h says.
 *
 * The last argument is a compile-time mask of the families to instantiate; a family left out costs nothing:
 *
 *   FVB_LANE_NOISE_AR1   AR(1) noise with one echo (the reference's noise=ar, num-echoes=1): four kernels, fed from the
 *                        float or the double tiles, with and without the free energy. Name: lane_ar1<NAME,P> /
 *                        lane_ar1<NAME,P,F>. No kernel reads the series in place: AR(1) refuses masked timepoints.
 *   FVB_LANE_NOISE_PHIS  white noise with 2 to 4 precisions (noise-pattern): two kernels, with 2 and with 4 moment sets
 *                        (3 precisions run the latter), that read the series in place - masked timepoints included - and
 *                        switch the free energy at run time. Name: lane_phis<NAME,P,2> / lane_phis<NAME,P,4>.
 *
 * The engine takes the route for a configuration when an entry for (name, n_params) with the family is registered, the
 * kernel variant is not `wave` and the conditions of the built-in models' kernels of that family hold: for a pattern at
 * most 32768 timepoints and the size rule of fabber_device_lane_model.h; for AR(1) no size rule (which of lane and wave
 * wins below a few thousand voxels under AR(1) has not been measured, for built-in or library models). Two echoes, cross
 * terms and 5 to 8 precisions run the wave kernels of FABBER_DEVICE_MODEL.
 *
 * The body is the struct of fabber_device_model.h, unchanged, and what fabber_device_lane_model.h says about
 * __forceinline__ holds here.
 *
 * The macro, at namespace scope:
 *   - instantiates the kernels of the families in the mask;
 *   - defines their launcher in this library's code object. The engine hands it the family, the moment sets of a pattern
 *     kernel, the feed and the dynamic LDS bytes of the launch (a pattern kernel's class bytes, one per timepoint): the
 *     launcher passes that count on and computes none. Asked for a family outside the mask, or for a feed the family has
 *     no kernel for, it answers -40 with a message and launches nothing;
 *   - registers { name, FVB_ABI_VERSION, sizeof(KernelArgs), P, mask, rows of each kernel's save buffer, launcher } with the
 *     engine from a static object whose destructor unregisters it. A refused registration (reported on stderr) leaves the
 *     model on the wave kernels.
 */
#ifndef FABBER_DEVICE_LANE_NOISE_MODEL_H
#define FABBER_DEVICE_LANE_NOISE_MODEL_H

#include "fabber_device_lane_model.h" /* fvb::LibraryLane: the body as a model of the lane kernels */
#include "../fabber_core_amd/csrc/vb_lane_ar_kernel.h"
#include "../fabber_core_amd/csrc/vb_lane_pattern_kernel.h"

namespace fvb
{
// The kernels of one macro line, looked up by what the engine asks for. A family outside FAMILIES is a discarded
// statement: its kernels are never instantiated.
template <class Eval, int P, int FAMILIES>
struct LibraryLaneNoise
{
    static_assert(P >= 1 && P <= 6, "FABBER_DEVICE_LANE_NOISE_MODEL: the lane kernels of a library body exist for 1 to 6 parameters");
    static_assert(FAMILIES != 0 && (FAMILIES & ~(FVB_LANE_NOISE_AR1 | FVB_LANE_NOISE_PHIS)) == 0,
        "FABBER_DEVICE_LANE_NOISE_MODEL: the mask names at least one of FVB_LANE_NOISE_AR1 and FVB_LANE_NOISE_PHIS and nothing else");
    typedef typename LibraryLane<Eval>::template Model<P> M;
    static constexpr bool ar1 = (FAMILIES & FVB_LANE_NOISE_AR1) != 0, phis = (FAMILIES & FVB_LANE_NOISE_PHIS) != 0;

    // (save_rows is the engine's business: it sized the buffer from the descriptor)
    static LaneKernelInfo kernels(int family, int pattern_n, bool need_f, const char *name)
    {
        LaneKernelInfo k{ nullptr, 0, name, nullptr, nullptr };
        if constexpr (ar1)
            if (family == FVB_LANE_NOISE_AR1)
            {
                k.fn_tiles_f32 = need_f ? vb_lane_ar_kernel<M, P, true, FEED_TILES_F32> : vb_lane_ar_kernel<M, P, false, FEED_TILES_F32>;
                k.fn_tiles_f64 = need_f ? vb_lane_ar_kernel<M, P, true, FEED_TILES_F64> : vb_lane_ar_kernel<M, P, false, FEED_TILES_F64>;
            }
        if constexpr (phis)
            if (family == FVB_LANE_NOISE_PHIS)
                k.fn = pattern_n == 2 ? vb_lane_pattern_kernel<M, P, 2> : (pattern_n == 4 ? vb_lane_pattern_kernel<M, P, 4> : nullptr);
        return k;
    }
    static constexpr int32_t save_rows_ar1()
    {
        if constexpr (ar1)
            return lane_ar_save_rows<P>();
        else
            return 0;
    }
    template <int N>
    static constexpr int32_t save_rows_phis()
    {
        if constexpr (phis)
            return lane_pattern_save_rows<P, N>();
        else
            return 0;
    }

    static int32_t launch(const char *model, const void *kernel_args, int32_t family, int32_t pattern_n, int32_t feed, uint32_t lds_bytes,
        void *stream, char *err, int32_t err_len)
    {
        const KernelArgs &ka = *static_cast<const KernelArgs *>(kernel_args);
        const bool need_f = ka.cfg.need_f != 0;
        const std::string of = std::string("<") + model + "," + std::to_string(P);
        const std::string name = family == FVB_LANE_NOISE_PHIS ? "lane_phis" + of + "," + std::to_string(pattern_n) + ">"
                                                                : "lane_ar1" + of + (need_f ? ",F>" : ">");
        if ((family != FVB_LANE_NOISE_AR1 && family != FVB_LANE_NOISE_PHIS) || (FAMILIES & family) == 0)
            return device_launch_result(-40, "lane kernels of device model '" + std::string(model) + "' with " + std::to_string(P)
                    + " parameters: not compiled with kernel family " + std::to_string(family) + " (its mask is " + std::to_string(FAMILIES) + ")",
                err, err_len);
        // (a feed without a kernel - AR(1) in place, a pattern from tiles, a pattern_n other than 2 and 4 - is a NULL entry:
        // launch_lane_kernel answers -40 for it and launches nothing)
        std::string msg;
        const int rc = launch_lane_kernel(kernels(family, pattern_n, need_f, name.c_str()), ka, feed, false, (size_t)lds_bytes,
            static_cast<hipStream_t>(stream), msg);
        return device_launch_result(rc, msg, err, err_len);
    }
};
} // namespace fvb

// (FVB_LANE_AR_CASE and FVB_LANE_PATTERN_CASE are the engine's own table entries of a built-in model: the same kernels,
// the same names)
#define FABBER_DEVICE_LANE_NOISE_MODEL(NAME, EVAL, NPARAMS, FAMILIES)                                                         \
    static int32_t FABBER_DEVICE_CAT(fabber_device_lane_noise_launch_, __LINE__)(const void *kernel_args, int32_t family,     \
        int32_t pattern_n, int32_t feed, uint32_t lds_bytes, void *stream, char *err, int32_t err_len)                        \
    {                                                                                                                         \
        return fvb::LibraryLaneNoise<EVAL, NPARAMS, (FAMILIES)>::launch(NAME, kernel_args, family, pattern_n, feed, lds_bytes, \
            stream, err, err_len);                                                                                            \
    }                                                                                                                         \
    static fvb::DeviceRegistration<fvb_device_lane_noise_model> FABBER_DEVICE_CAT(fabber_device_lane_noise_registration_, __LINE__)( \
        fvb_device_lane_noise_model{ NAME, FVB_ABI_VERSION, (uint32_t)sizeof(fvb::KernelArgs), NPARAMS, (FAMILIES),            \
            fvb::LibraryLaneNoise<EVAL, NPARAMS, (FAMILIES)>::save_rows_ar1(),                                                \
            fvb::LibraryLaneNoise<EVAL, NPARAMS, (FAMILIES)>::save_rows_phis<2>(),                                            \
            fvb::LibraryLaneNoise<EVAL, NPARAMS, (FAMILIES)>::save_rows_phis<4>(),                                            \
            &FABBER_DEVICE_CAT(fabber_device_lane_noise_launch_, __LINE__) },                                                 \
        NPARAMS, &fabber_vb_register_device_lane_noise_model, &fabber_vb_unregister_device_lane_noise_model,                  \
        "AR(1) / noise-pattern lane kernels of ", "the model runs on the wave kernels under these noise models");

#endif /* FABBER_DEVICE_LANE_NOISE_MODEL_H */
