/*
 * fabber_device_registration.h - what the headers that compile the engine's kernels around a model library's device
 * body share (fabber_device_model.h, fabber_device_lane_model.h, fabber_device_lane_noise_model.h, fabber_device_nlls_model.h,
 * fabber_device_spatial_model.h, fabber_device_spatial_noise_model.h, fabber_device_spatial_wave_model.h, fabber_device_spatial_wave_noise_model.h, fabber_device_spatial_wave_ar_model.h, fabber_device_results_model.h, fabber_device_init_model.h): the static object that registers an entry with the engine, the token pasting of
 * their macros and the way a launcher hands its error text back. A library includes those headers, not this one.
 */
#ifndef FABBER_DEVICE_REGISTRATION_H
#define FABBER_DEVICE_REGISTRATION_H

#include "fabber_vb.h"

#include <cstdio>
#include <cstring>
#include <string>

namespace fvb
{
// Holds the descriptor, registers it in its constructor and unregisters it in its destructor if the engine took it (the
// library's static object). n_params: the parameter count of the entry's key, 0 = it has none.
template <class Descriptor>
struct DeviceRegistration
{
    Descriptor descriptor;
    int32_t n_params;
    int32_t (*remove)(const char *name, int32_t n_params);
    bool registered;
    // a refusal goes to stderr: "fabber: WHATdevice model 'NAME' (N parameters) not registered (the engine's reason): OTHERWISE"
    DeviceRegistration(const Descriptor &d, int32_t n_params_, int32_t (*add)(const Descriptor *), int32_t (*remove_)(const char *, int32_t),
        const char *what, const char *otherwise)
        : descriptor(d), n_params(n_params_), remove(remove_)
    {
        registered = add(&descriptor) == 0;
        if (!registered)
            fprintf(stderr, "fabber: %sdevice model '%s'%s not registered (%s): %s\n", what, descriptor.name,
                n_params ? (" (" + std::to_string(n_params) + " parameters)").c_str() : "", fabber_vb_last_error(), otherwise);
    }
    ~DeviceRegistration()
    {
        if (registered)
            (void)remove(descriptor.name, n_params);
    }
    DeviceRegistration(const DeviceRegistration &) = delete;
    DeviceRegistration &operator=(const DeviceRegistration &) = delete;
};

// what a launcher answers: rc, and its message in err / err_len where it failed
inline int32_t device_launch_result(int rc, const std::string &msg, char *err, int32_t err_len)
{
    if (rc && err && err_len > 0)
    {
        strncpy(err, msg.c_str(), (size_t)err_len - 1);
        err[err_len - 1] = 0;
    }
    return rc;
}
} // namespace fvb

#define FABBER_DEVICE_CAT2(a, b) a##b
#define FABBER_DEVICE_CAT(a, b) FABBER_DEVICE_CAT2(a, b)

#endif /* FABBER_DEVICE_REGISTRATION_H */
