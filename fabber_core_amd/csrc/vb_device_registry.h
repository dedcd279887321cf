/*
 * vb_device_registry.h - the registries of what model libraries compile around their device bodies
 * (include/fabber_device_*model.h): one class template over the descriptor type, the checks every registration shares,
 * and what the entry points ask about a configuration that names such a body (FVB_MODEL_PLUGIN). The extern "C"
 * functions stay with the kernels they register (vb_api.hip, vb_nlls.hip, vb_spatial_api.hip): each is one call into
 * the template. No kernel includes this file.
 */
#pragma once

#include "vb_host_stage.h"

#include <cstring>
#include <mutex>
#include <string>
#include <vector>

namespace fvb
{
// One struct whose size a library reports in its descriptor, against the engine's own
struct DeviceStructSize
{
    const char *label;
    uint32_t library;
    size_t engine;
};

// What tells one descriptor type from another, specialised next to its extern "C" functions:
//   noun          "device lane model": how the messages call a descriptor
//   first_code    the first of the five consecutive error codes: bad descriptor / name / parameter count, then -1 ABI
//                 version, -2 struct sizes, -3 already registered, -4 not registered
//   sizes(m)      the struct sizes m reports, with their labels
//   bad_params(m) why m's parameter count has no kernels (NULL: it has)
//   entry(name, n_params), is   how the messages call one entry, with its verb ("is" / "are")
//   absent(name, n_params)      what unregistering an entry that is not there is told
//   absent_code   (optional) the code for "not registered" where first_code - 4 is taken by something else
template <class D> struct DeviceRegistryTraits;

template <class Tr> constexpr auto device_registry_absent_code(int) -> decltype(Tr::absent_code)
{
    return Tr::absent_code;
}
template <class Tr> constexpr int device_registry_absent_code(long)
{
    return Tr::first_code - 4;
}

// The key of an entry is (name, parameter count); the descriptors of the wave body, of the result-image kernel and of
// the initial-posterior kernel have no count, nor have the wave-per-voxel spatial kernels (a runtime value there): 0
inline int registered_params(const fvb_device_model &)
{
    return 0;
}
inline int registered_params(const fvb_device_spatial_wave_model &)
{
    return 0;
}
inline int registered_params(const fvb_device_spatial_wave_noise_model &)
{
    return 0;
}
inline int registered_params(const fvb_device_spatial_wave_ar_model &)
{
    return 0;
}
inline int registered_params(const fvb_device_init_model &)
{
    return 0;
}
inline int registered_params(const fvb_device_results_model &)
{
    return 0;
}
template <class D> int registered_params(const D &m)
{
    return m.n_params;
}

// The descriptors are the libraries' own static objects: they stay valid until the library unregisters them (the
// destructor of the object that registered them does).
template <class D> class DeviceRegistry
{
public:
    // one per descriptor type and engine library (never destroyed: libraries unregister from static destructors)
    static DeviceRegistry &instance()
    {
        static DeviceRegistry *r = new DeviceRegistry;
        return *r;
    }

    int add(const D *model)
    {
        using Tr = DeviceRegistryTraits<D>;
        const std::string noun = Tr::noun;
        if (!model || !model->name || !model->name[0] || !model->launch)
            return api_fail(Tr::first_code, "registering a " + noun + ": descriptor, name or launcher is NULL");
        const std::string name = model->name, who = noun + " '" + name + "': ";
        if (name.size() >= FVB_DEVICE_MODEL_NAME_MAX)
            return api_fail(Tr::first_code, who + "the name is longer than " + std::to_string(FVB_DEVICE_MODEL_NAME_MAX - 1) + " characters");
        if (model->abi_version != FVB_ABI_VERSION)
            return api_fail(Tr::first_code - 1, noun + " '" + name + "' was built for ABI version " + std::to_string(model->abi_version)
                    + ", the engine is version " + std::to_string(FVB_ABI_VERSION));
        std::string sizes;
        bool sizes_differ = false;
        for (const DeviceStructSize &s : Tr::sizes(*model))
        {
            sizes += (sizes.empty() ? "" : ", ") + std::string(s.label) + " " + std::to_string(s.library) + " against " + std::to_string(s.engine)
                + (sizes.empty() ? " bytes" : "");
            sizes_differ |= s.library != s.engine;
        }
        if (sizes_differ)
            return api_fail(Tr::first_code - 2, who + "struct size mismatch (" + sizes + "): the library was compiled against other kernel headers");
        const int n_params = registered_params(*model);
        if (const char *why = Tr::bad_params(*model))
            return api_fail(Tr::first_code, who + std::to_string(n_params) + " parameters (" + why + ")");
        std::lock_guard<std::mutex> hold(lock_);
        if (at(name.c_str(), n_params) < models_.size())
            return api_fail(Tr::first_code - 3, Tr::entry(name, n_params) + " " + Tr::is + " already registered");
        models_.push_back(model);
        return 0;
    }

    int remove(const char *name, int n_params)
    {
        using Tr = DeviceRegistryTraits<D>;
        if (!name)
            return api_fail(Tr::first_code, "unregistering a " + std::string(Tr::noun) + ": name is NULL");
        std::lock_guard<std::mutex> hold(lock_);
        const size_t i = at(name, n_params);
        if (i == models_.size())
            return api_fail(device_registry_absent_code<Tr>(0), Tr::absent(name, n_params));
        models_.erase(models_.begin() + (long)i);
        return 0;
    }

    int32_t count()
    {
        std::lock_guard<std::mutex> hold(lock_);
        return (int32_t)models_.size();
    }
    const char *name(int32_t i)
    {
        std::lock_guard<std::mutex> hold(lock_);
        return (i >= 0 && (size_t)i < models_.size()) ? models_[(size_t)i]->name : nullptr;
    }
    int32_t params(int32_t i, int32_t none)
    {
        std::lock_guard<std::mutex> hold(lock_);
        return (i >= 0 && (size_t)i < models_.size()) ? registered_params(*models_[(size_t)i]) : none;
    }

    // entry (optional): the descriptor, copied while the registry is locked - a descriptor may be unregistered by
    // another thread at any time; the library itself must stay loaded while a run that uses its kernels is under way
    bool find(const std::string &name, int n_params, D *entry = nullptr)
    {
        std::lock_guard<std::mutex> hold(lock_);
        const size_t i = at(name.c_str(), n_params);
        if (i < models_.size() && entry)
            *entry = *models_[i];
        return i < models_.size();
    }

private:
    size_t at(const char *name, int n_params) const // (locked by the caller) models_.size(): no such entry
    {
        size_t i = 0;
        while (i < models_.size() && !(registered_params(*models_[i]) == n_params && strcmp(models_[i]->name, name) == 0))
            i++;
        return i;
    }
    std::mutex lock_;
    std::vector<const D *> models_;
};

// the wave-per-voxel body of a name (include/fabber_device_model.h): what every other entry of the name is looked up after
inline bool find_wave_body(const std::string &name, fvb_device_model *entry = nullptr)
{
    return DeviceRegistry<fvb_device_model>::instance().find(name, 0, entry);
}

// the name as a configuration carries it: not necessarily terminated
inline std::string config_device_model(const fvb_config *cfg)
{
    return std::string(cfg->device_model, strnlen(cfg->device_model, sizeof(cfg->device_model)));
}

// the initial-posterior kernel of the body a configuration names (include/fabber_device_init_model.h): an entry counts
// next to a wave body of its name
inline bool find_init_entry(const fvb_config *cfg, fvb_device_init_model *entry = nullptr)
{
    if (cfg->model != FVB_MODEL_PLUGIN)
        return false;
    const std::string name = config_device_model(cfg);
    return find_wave_body(name) && DeviceRegistry<fvb_device_init_model>::instance().find(name, 0, entry);
}

// A run of such a body without cfg->init_mvn: the entry's kernel writes the image into `image` (device memory, the rows
// of the configuration's MVN) on the run's stream, ahead of everything that reads it. 0, or the code with its message.
inline int launch_init_entry(const fvb_device_init_model &entry, const fvb_config *cfg, const void *data, double *image, hipStream_t stream)
{
    char err[256] = "";
    const int rc = entry.launch(cfg, data, image, (void *)stream, err, (int32_t)sizeof(err));
    return rc ? api_fail(rc, "initial-posterior kernel of the device model '" + config_device_model(cfg) + "': " + err) : 0;
}

// the argument checks of a configuration with FVB_MODEL_PLUGIN
inline int check_device_model_config(const fvb_config *cfg)
{
    const std::string name = config_device_model(cfg);
    if (name.empty())
        return api_fail(-16, "FVB_MODEL_PLUGIN needs the name of a registered device model (fvb_config.device_model)");
    if (!find_wave_body(name))
        return api_fail(-16, "no device model '" + name + "' is registered (fabber_vb_register_device_model)");
    if (cfg->n_model_consts < 0 || (cfg->n_model_consts > 0 && !cfg->model_consts))
        return api_fail(-17, "device model '" + name + "': n_model_consts constants announced but model_consts is NULL");
    if (cfg->n_model_supp < 0 || (cfg->n_model_supp > 0 && !cfg->model_supp))
        return api_fail(-17, "device model '" + name + "': n_model_supp rows of supplementary data announced but model_supp is NULL");
    return 0;
}
} // namespace fvb
