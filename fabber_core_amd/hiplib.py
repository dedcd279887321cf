"""ctypes binding of fabber_core_amd/lib/libfabber_vb_hip.so (the HIP voxelwise-VB engine).

There is deliberately no fallback: if the shared library is missing or no GPU is visible the
functions raise. Build the library with ``python -m fabber_core_amd.build``.
"""
import ctypes as C
import os

import numpy as np

from . import vbabi

_HERE = os.path.dirname(os.path.abspath(__file__))
# (FVB_LIB_PATH: an experiment build of the engine, see fabber_core_amd/build.py --variant)
LIB_PATH = os.environ.get("FVB_LIB_PATH") or os.path.join(_HERE, "lib", "libfabber_vb_hip.so")
_LIB = None


# The registries of what model libraries compile around their device bodies (fabber_vb.h): the kind as the C functions
# spell it, the descriptor class, and whether an entry's key carries a parameter count next to the name
_DEVICE_ENTRIES = (("device_model", vbabi.FvbDeviceModel, False),
                   ("device_lane_model", vbabi.FvbDeviceLaneModel, True),
                   ("device_lane_noise_model", vbabi.FvbDeviceLaneNoiseModel, True),
                   ("device_nlls_model", vbabi.FvbDeviceNllsModel, True),
                   ("device_spatial_model", vbabi.FvbDeviceSpatialModel, True),
                   ("device_spatial_noise_model", vbabi.FvbDeviceSpatialNoiseModel, True),
                   ("device_spatial_wave_model", vbabi.FvbDeviceSpatialWaveModel, False),
                   ("device_spatial_wave_noise_model", vbabi.FvbDeviceSpatialWaveNoiseModel, False),
                   ("device_spatial_wave_ar_model", vbabi.FvbDeviceSpatialWaveArModel, False),
                   ("device_results_model", vbabi.FvbDeviceResultsModel, False),
                   ("device_init_model", vbabi.FvbDeviceInitModel, False))


class HipEngineError(RuntimeError):
    pass


def available():
    """True if the native library has been built (says nothing about a GPU being present)."""
    return os.path.exists(LIB_PATH)


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise HipEngineError("%s not built: run `python -m fabber_core_amd.build` (no CPU fallback exists)" % LIB_PATH)
        from . import single_hip_runtime
        single_hip_runtime()
        L = C.CDLL(LIB_PATH)
        cfgp, outp, ppp = C.POINTER(vbabi.FvbConfig), C.POINTER(vbabi.FvbOutputs), C.POINTER(vbabi.FvbPostproc)
        L.fabber_vb_mvn_rows.restype = C.c_int32
        L.fabber_vb_mvn_rows.argtypes = [C.c_int32]
        L.fabber_vb_abi_version.restype = C.c_int32
        L.fabber_vb_device_count.restype = C.c_int32
        L.fabber_vb_last_error.restype = C.c_char_p
        L.fabber_vb_kernel_name.restype = C.c_char_p
        L.fabber_vb_kernel_name.argtypes = [cfgp]
        L.fabber_vb_set_variant.argtypes = [C.c_int32]
        L.fabber_vb_set_residual_mode.argtypes = [C.c_int32]
        L.fabber_vb_set_residual_tolerance.argtypes = [C.c_double]
        L.fabber_vb_run_device.restype = C.c_int32
        L.fabber_vb_run_device.argtypes = [cfgp, C.c_void_p, outp, C.c_void_p]
        L.fabber_vb_run_device_ex.restype = C.c_int32
        L.fabber_vb_run_device_ex.argtypes = [cfgp, C.c_void_p, outp, C.c_void_p, C.c_int32]
        L.fabber_vb_run_host.restype = C.c_int32
        L.fabber_vb_run_host.argtypes = [cfgp, C.c_void_p, outp, C.c_int32]
        L.fabber_vb_run_host_multi.restype = C.c_int32
        L.fabber_vb_run_host_multi.argtypes = [cfgp, C.c_void_p, outp, C.POINTER(C.c_int32), C.c_int32, C.POINTER(vbabi.FvbSummary)]
        L.fabber_vb_postproc_device.restype = C.c_int32
        L.fabber_vb_postproc_device.argtypes = [cfgp, C.c_void_p, C.c_void_p, ppp, C.c_void_p]
        L.fabber_vb_postproc_host.restype = C.c_int32
        L.fabber_vb_postproc_host.argtypes = [cfgp, C.c_void_p, C.c_void_p, ppp, C.c_int32]
        L.fabber_vb_convergence_trace.restype = C.c_int32
        L.fabber_vb_convergence_trace.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_int32,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        for name in ("fabber_vb_gammaln", "fabber_vb_digamma", "fabber_vb_exp_acc"):
            getattr(L, name).restype = C.c_double
            getattr(L, name).argtypes = [C.c_double]
        L.fabber_vb_transform.restype = C.c_double
        L.fabber_vb_transform.argtypes = [C.c_int32, C.c_int32, C.c_double]
        L.fabber_vb_ldl_inverse.restype = C.c_int32
        L.fabber_vb_ldl_inverse.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fabber_nlls_run_host.restype = C.c_int32
        L.fabber_nlls_run_host.argtypes = [cfgp, C.POINTER(vbabi.FvbNlls), C.c_void_p, outp, C.c_int32]
        L.fabber_nlls_run_device.restype = C.c_int32
        L.fabber_nlls_run_device.argtypes = [cfgp, C.POINTER(vbabi.FvbNlls), C.c_void_p, outp, C.c_void_p, C.c_int32]
        L.fabber_nlls_defaults.restype = None
        L.fabber_nlls_defaults.argtypes = [C.POINTER(vbabi.FvbNlls)]
        for kind, descriptor, keyed in _DEVICE_ENTRIES:
            def fn(what):
                return getattr(L, "fabber_vb_" + what.replace("KIND", kind))
            fn("register_KIND").restype = C.c_int32
            fn("register_KIND").argtypes = [C.POINTER(descriptor)]
            fn("unregister_KIND").restype = C.c_int32
            fn("unregister_KIND").argtypes = [C.c_char_p] + [C.c_int32] * keyed
            fn("KIND_count").restype = C.c_int32
            fn("KIND_name").restype = C.c_char_p
            fn("KIND_name").argtypes = [C.c_int32]
            if keyed:
                fn("KIND_params").restype = C.c_int32
                fn("KIND_params").argtypes = [C.c_int32]
        L.fabber_vb_find_device_lane_noise_model.restype = C.c_int32
        L.fabber_vb_find_device_lane_noise_model.argtypes = [C.c_char_p, C.c_int32, C.POINTER(vbabi.FvbDeviceLaneNoiseModel)]
        L.fabber_vb_find_device_spatial_noise_model.restype = C.c_int32
        L.fabber_vb_find_device_spatial_noise_model.argtypes = [C.c_char_p, C.c_int32, C.POINTER(vbabi.FvbDeviceSpatialNoiseModel)]
        L.fabber_vb_find_device_spatial_wave_model.restype = C.c_int32
        L.fabber_vb_find_device_spatial_wave_model.argtypes = [C.c_char_p, C.POINTER(vbabi.FvbDeviceSpatialWaveModel)]
        L.fabber_vb_find_device_spatial_wave_noise_model.restype = C.c_int32
        L.fabber_vb_find_device_spatial_wave_noise_model.argtypes = [C.c_char_p, C.POINTER(vbabi.FvbDeviceSpatialWaveNoiseModel)]
        L.fabber_vb_find_device_spatial_wave_ar_model.restype = C.c_int32
        L.fabber_vb_find_device_spatial_wave_ar_model.argtypes = [C.c_char_p, C.POINTER(vbabi.FvbDeviceSpatialWaveArModel)]
        L.fabber_nlls_kernel_name.restype = C.c_char_p
        L.fabber_nlls_kernel_name.argtypes = [cfgp]
        L.fabber_vb_spatial_kernel_name.restype = C.c_char_p
        L.fabber_vb_spatial_kernel_name.argtypes = [cfgp]
        L.fabber_vb_postproc_kernel_name.restype = C.c_char_p
        L.fabber_vb_postproc_kernel_name.argtypes = [cfgp]
        L.fabber_vb_init_posterior_kernel_name.restype = C.c_char_p
        L.fabber_vb_init_posterior_kernel_name.argtypes = [cfgp]
        L.fabber_vb_init_posterior_device.restype = C.c_int32
        L.fabber_vb_init_posterior_device.argtypes = [cfgp, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fabber_vb_init_posterior_host.restype = C.c_int32
        L.fabber_vb_init_posterior_host.argtypes = [cfgp, C.c_void_p, C.c_void_p, C.c_int32]
        if L.fabber_vb_abi_version() != vbabi.FVB_ABI_VERSION:
            raise HipEngineError("libfabber_vb_hip.so ABI version mismatch: rebuild")
        _LIB = L
    return _LIB


def _check(rc):
    if rc != 0:
        raise HipEngineError("fabber_vb error %d: %s" % (rc, lib().fabber_vb_last_error().decode()))


def device_count():
    return lib().fabber_vb_device_count()


_MODEL_LIBRARIES = {}


def load_model_library(path):
    """Open a model library that carries device bodies (include/fabber_device_model.h): its static objects register
    them with the engine, after which build_config(MODEL_PLUGIN, device_model=name) can name them. The engine is
    loaded first and both are opened with RTLD_GLOBAL, so that the library finds the engine's registry. Returns the
    ctypes handle; a library is opened once per process."""
    path = os.path.abspath(path)
    if path not in _MODEL_LIBRARIES:
        lib()
        C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)  # (the same handle, its symbols now visible to what is opened next)
        _MODEL_LIBRARIES[path] = C.CDLL(path, mode=C.RTLD_GLOBAL)
    return _MODEL_LIBRARIES[path]


def _listed(kind, keyed):
    L = lib()
    names = [getattr(L, "fabber_vb_%s_name" % kind)(i).decode() for i in range(getattr(L, "fabber_vb_%s_count" % kind)())]
    return [(n, getattr(L, "fabber_vb_%s_params" % kind)(i)) for i, n in enumerate(names)] if keyed else names


def _register(kind, descriptor):
    _check(getattr(lib(), "fabber_vb_register_" + kind)(C.byref(descriptor)))


def _unregister(kind, name, *n_params):
    _check(getattr(lib(), "fabber_vb_unregister_" + kind)(name.encode(), *n_params))


def device_models():
    """Names of the device bodies registered with the engine."""
    return _listed("device_model", False)


def register_device_model(descriptor):
    """fabber_vb_register_device_model with a vbabi.FvbDeviceModel (the caller keeps it alive); raises with the engine's
    message when the registration is refused. The six below: the same with the descriptor class of their kind."""
    _register("device_model", descriptor)


def unregister_device_model(name):
    _unregister("device_model", name)


def device_lane_models():
    """(name, parameter count) of the lane-kernel entries registered with the engine (include/fabber_device_lane_model.h)."""
    return _listed("device_lane_model", True)


def register_device_lane_model(descriptor):
    _register("device_lane_model", descriptor)


def unregister_device_lane_model(name, n_params):
    _unregister("device_lane_model", name, n_params)


def device_lane_noise_models():
    """(name, parameter count) of the AR(1) / noise-pattern lane-kernel entries registered with the engine
    (include/fabber_device_lane_noise_model.h)."""
    return _listed("device_lane_noise_model", True)


def register_device_lane_noise_model(descriptor):
    _register("device_lane_noise_model", descriptor)


def unregister_device_lane_noise_model(name, n_params):
    _unregister("device_lane_noise_model", name, n_params)


def find_device_lane_noise_model(name, n_params):
    """a copy of the entry for (name, n_params) - families, rows of the save buffers, launcher - or None"""
    entry = vbabi.FvbDeviceLaneNoiseModel()
    return entry if lib().fabber_vb_find_device_lane_noise_model(name.encode(), n_params, C.byref(entry)) else None


def device_nlls_models():
    """(name, parameter count) of the NLLS minimisers registered with the engine (include/fabber_device_nlls_model.h);
    a count of 0 is the wave-per-voxel minimiser."""
    return _listed("device_nlls_model", True)


def register_device_nlls_model(descriptor):
    _register("device_nlls_model", descriptor)


def unregister_device_nlls_model(name, n_params):
    _unregister("device_nlls_model", name, n_params)


def device_spatial_models():
    """(name, parameter count) of the spatial-VB entries registered with the engine (include/fabber_device_spatial_model.h)."""
    return _listed("device_spatial_model", True)


def register_device_spatial_model(descriptor):
    _register("device_spatial_model", descriptor)


def unregister_device_spatial_model(name, n_params):
    _unregister("device_spatial_model", name, n_params)


def device_spatial_noise_models():
    """(name, parameter count) of the AR(1) / noise-pattern spatial-VB entries registered with the engine
    (include/fabber_device_spatial_noise_model.h)."""
    return _listed("device_spatial_noise_model", True)


def register_device_spatial_noise_model(descriptor):
    _register("device_spatial_noise_model", descriptor)


def unregister_device_spatial_noise_model(name, n_params):
    _unregister("device_spatial_noise_model", name, n_params)


def find_device_spatial_noise_model(name, n_params):
    """a copy of the entry for (name, n_params) - families, rows of the state images, launcher - or None"""
    entry = vbabi.FvbDeviceSpatialNoiseModel()
    return entry if lib().fabber_vb_find_device_spatial_noise_model(name.encode(), n_params, C.byref(entry)) else None


def device_spatial_wave_models():
    """Names of the wave-per-voxel spatial-VB entries registered with the engine (include/fabber_device_spatial_wave_model.h):
    any parameter count up to FVB_MAX_PARAMS."""
    return _listed("device_spatial_wave_model", False)


def register_device_spatial_wave_model(descriptor):
    _register("device_spatial_wave_model", descriptor)


def unregister_device_spatial_wave_model(name):
    _unregister("device_spatial_wave_model", name)


def find_device_spatial_wave_model(name):
    """a copy of the entry of `name` - the sizes and the LDS probe it reported, launcher - or None"""
    entry = vbabi.FvbDeviceSpatialWaveModel()
    return entry if lib().fabber_vb_find_device_spatial_wave_model(name.encode(), C.byref(entry)) else None


def device_spatial_wave_noise_models():
    """Names of the wave-per-voxel spatial-VB entries for noise patterns registered with the engine
    (include/fabber_device_spatial_wave_noise_model.h): any parameter count up to FVB_MAX_PARAMS, 2 to FVB_MAX_PHIS precisions."""
    return _listed("device_spatial_wave_noise_model", False)


def register_device_spatial_wave_noise_model(descriptor):
    _register("device_spatial_wave_noise_model", descriptor)


def unregister_device_spatial_wave_noise_model(name):
    _unregister("device_spatial_wave_noise_model", name)


def find_device_spatial_wave_noise_model(name):
    """a copy of the entry of `name` - the sizes and the LDS probe it reported, its families mask, launcher - or None"""
    entry = vbabi.FvbDeviceSpatialWaveNoiseModel()
    return entry if lib().fabber_vb_find_device_spatial_wave_noise_model(name.encode(), C.byref(entry)) else None


def device_spatial_wave_ar_models():
    """Names of the wave-per-voxel spatial-VB entries for AR(1) noise registered with the engine
    (include/fabber_device_spatial_wave_ar_model.h): any parameter count up to FVB_MAX_PARAMS, one echo, no cross terms."""
    return _listed("device_spatial_wave_ar_model", False)


def register_device_spatial_wave_ar_model(descriptor):
    _register("device_spatial_wave_ar_model", descriptor)


def unregister_device_spatial_wave_ar_model(name):
    _unregister("device_spatial_wave_ar_model", name)


def find_device_spatial_wave_ar_model(name):
    """a copy of the entry of `name` - the sizes and the LDS probe it reported, its launcher - or None"""
    entry = vbabi.FvbDeviceSpatialWaveArModel()
    return entry if lib().fabber_vb_find_device_spatial_wave_ar_model(name.encode(), C.byref(entry)) else None


def device_results_models():
    """Names of the result-image kernels registered with the engine (include/fabber_device_results_model.h)."""
    return _listed("device_results_model", False)


def register_device_results_model(descriptor):
    _register("device_results_model", descriptor)


def unregister_device_results_model(name):
    _unregister("device_results_model", name)


def device_init_models():
    """Names of the initial-posterior kernels registered with the engine (include/fabber_device_init_model.h)."""
    return _listed("device_init_model", False)


def register_device_init_model(descriptor):
    _register("device_init_model", descriptor)


def unregister_device_init_model(name):
    _unregister("device_init_model", name)


def find_device_init_model(name):
    """True where an initial-posterior kernel of that name is registered (it is used next to a wave body of the name)"""
    return name in device_init_models()


def kernel_name(holder):
    return lib().fabber_vb_kernel_name(C.byref(holder.cfg)).decode()


def postproc_kernel_name(holder):
    """Where postproc_host / postproc_device take model fit and residuals from: "postproc" (a built-in model),
    "postproc<NAME>" (the kernel a model library compiled around its body), or "" where a request for either image is
    refused (-85: a library body without a results entry)."""
    return lib().fabber_vb_postproc_kernel_name(C.byref(holder.cfg)).decode()


def nlls_kernel_name(holder):
    """The kernel nlls_run_host would take: "nlls<exp,2>", "nlls<NAME,P>", "nlls_wave", "nlls_wave<NAME>", or "" where the
    run would be refused (a model without a device body, a library body without an NLLS entry)."""
    return lib().fabber_nlls_kernel_name(C.byref(holder.cfg)).decode()


def spatial_kernel_name(holder):
    """The kernel table run_spatial_host would take: "spatial<exp,2>", "spatial<NAME,P>", ..., or "" where the run would
    answer -40 or -44 (no kernels for the model / parameter count / noise model, a library body without a spatial entry)."""
    return lib().fabber_vb_spatial_kernel_name(C.byref(holder.cfg)).decode()


def set_variant(variant):
    lib().fabber_vb_set_variant({"auto": 0, "lane": 1, "wave": 2}.get(variant, variant))


def set_residual_mode(mode):
    """k'Qk: 'auto' (moments + exact fallback), 'exact' (always direct), 'moments' (never)."""
    lib().fabber_vb_set_residual_mode({"auto": 0, "exact": 1, "moments": 2}.get(mode, mode))


def set_residual_tolerance(tol):
    lib().fabber_vb_set_residual_tolerance(float(tol))


def n_unmasked(holder):
    phi = holder.keep.get("phi_index")
    return int(holder.cfg.n_times if phi is None else np.count_nonzero(phi != 255))


def _prepare_data(holder, data):
    cfg = holder.cfg
    data = np.ascontiguousarray(data)
    if data.dtype == np.float64:
        cfg.data_f64 = 1
    else:
        data = np.ascontiguousarray(data, dtype=np.float32)
        cfg.data_f64 = 0
    assert data.shape == (cfg.n_times, cfg.n_voxels), (data.shape, cfg.n_times, cfg.n_voxels)
    return data


def run_host(holder, data, device=0, devices=None, into=None):
    """Voxelwise VB on the GPU from host arrays (config pointers are host numpy arrays).
    Returns the same dict of arrays as tests/oracle.py:run. devices: "all" or a list of device indices
    (fabber_vb_run_host_multi: contiguous voxel blocks, one per entry); the result then also holds
    `summary` = (sum of F, sum of iterations, bad voxels). into: the dict a previous call returned - its arrays are
    written again instead of new ones being allocated and filled (176 MB per million voxels of the bi-exponential
    configuration: as long as the engine's share of the call)."""
    cfg = holder.cfg
    data = _prepare_data(holder, data)
    V = cfg.n_voxels
    if into is not None:
        arrs = {k: into[k] for k in ("mvn", "free_energy", "status", "iterations", "f_history_len", "f_history") if k in into}
    else:
        arrs = dict(
            mvn=np.full((holder.n_mvn_rows, V), np.nan),
            free_energy=np.full(V, np.nan),
            status=np.full(V, -1, dtype=np.int32),
            iterations=np.full(V, -1, dtype=np.int32),
            f_history_len=np.zeros(V, dtype=np.int32),
        )
        if cfg.f_history_rows > 0:
            arrs["f_history"] = np.full((cfg.f_history_rows, V), np.nan)
    out = vbabi.FvbOutputs()
    for k, a in arrs.items():
        setattr(out, k, a.ctypes.data)
    if devices is None:
        _check(lib().fabber_vb_run_host(C.byref(cfg), data.ctypes.data, C.byref(out), device))
    else:
        summary = vbabi.FvbSummary()
        if devices == "all":
            _check(lib().fabber_vb_run_host_multi(C.byref(cfg), data.ctypes.data, C.byref(out), None, 0, C.byref(summary)))
        else:
            ids = (C.c_int32 * len(devices))(*devices)
            _check(lib().fabber_vb_run_host_multi(C.byref(cfg), data.ctypes.data, C.byref(out), ids, len(devices), C.byref(summary)))
        arrs["summary"] = (summary.sum_free_energy, summary.sum_iterations, summary.bad_voxels)
    arrs["setup_failed"] = (arrs["status"] & 0x100) != 0
    arrs["status"] = arrs["status"] & 0xFF
    return arrs


def nlls_run_host(holder, data, lm=False, start=None, settings=None, device=0):
    """method=nlls on the GPU from host arrays. `start` = Fabber-space starting estimate
    (default zeros, what the built-in models' HardcodedInitialDists leaves). Returns mvn
    [mvn_rows(P)][V] (parameters only), status, iterations, cost (final sum of squares)."""
    cfg = holder.cfg
    data = _prepare_data(holder, data)
    V, P = cfg.n_voxels, cfg.n_params
    holder.set_post_mean([0.0] * P if start is None else start)
    nl = settings or vbabi.FvbNlls.defaults(lm)
    arrs = dict(mvn=np.full((vbabi.mvn_rows(P), V), np.nan), status=np.full(V, -1, dtype=np.int32),
                iterations=np.full(V, -1, dtype=np.int32), free_energy=np.full(V, np.nan))
    out = vbabi.FvbOutputs()
    for k, a in arrs.items():
        setattr(out, k, a.ctypes.data)
    _check(lib().fabber_nlls_run_host(C.byref(cfg), C.byref(nl), data.ctypes.data, C.byref(out), device))
    arrs["cost"] = arrs.pop("free_energy")
    return arrs


LINEARISE_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double))


def recentre_callback(model, T, P):
    """fvb_linearise_fn from a Python model: model(params [n][P] Fabber space, voxel ids [n]) -> [n][T]. The offset and
    the Jacobian as LinearizedFwdModel::ReCentre computes them (fwdmodel_linear.cc:126-182): central differences,
    delta = max(|centre| 1e-5, 1e-10). Keep the returned object alive for the duration of the call."""
    def cb(user, n, ids, means, lin):
        try:
            v = np.ctypeslib.as_array(ids, (n,))
            m = np.ctypeslib.as_array(means, (n * P,)).reshape(n, P)
            out = np.ctypeslib.as_array(lin, (n * T * (P + 1),)).reshape(n, T * (P + 1))
            out[:, :T] = model(m, v)
            J = np.empty((n, T, P))
            for i in range(P):
                delta = np.maximum(np.abs(m[:, i] * 1e-5), 1e-10)
                up, dn = m.copy(), m.copy()
                up[:, i] = m[:, i] + delta
                dn[:, i] = m[:, i] - delta
                J[:, :, i] = (model(up, v) - model(dn, v)) / (up[:, i] - dn[:, i])[:, None]
            out[:, T:] = J.reshape(n, -1)
            return 0
        except Exception:  # noqa: BLE001 (the engine reports -54)
            return 1
    return LINEARISE_FN(cb)


def nlls_run_hostmodel_host(holder, data, model, lm=False, start=None, settings=None, device=0):
    """method=nlls with the model evaluated by the caller (fabber_nlls_run_hostmodel_host): `model` as for
    recentre_callback. The holder's model fields are not read."""
    cfg = holder.cfg
    data = _prepare_data(holder, data)
    V, P, T = cfg.n_voxels, cfg.n_params, cfg.n_times
    holder.set_post_mean([0.0] * P if start is None else start)
    nl = settings or vbabi.FvbNlls.defaults(lm)
    arrs = dict(mvn=np.full((vbabi.mvn_rows(P), V), np.nan), status=np.full(V, -1, dtype=np.int32),
                iterations=np.full(V, -1, dtype=np.int32), free_energy=np.full(V, np.nan))
    out = vbabi.FvbOutputs()
    for k, a in arrs.items():
        setattr(out, k, a.ctypes.data)
    cb = recentre_callback(model, T, P)
    L = lib()
    L.fabber_nlls_run_hostmodel_host.restype = C.c_int32
    L.fabber_nlls_run_hostmodel_host.argtypes = [C.POINTER(vbabi.FvbConfig), C.POINTER(vbabi.FvbNlls), C.c_void_p,
                                                 C.POINTER(vbabi.FvbOutputs), C.c_int32, LINEARISE_FN, C.c_void_p]
    saved = cfg.model
    cfg.model = vbabi.MODEL_HOSTJAC
    try:
        _check(L.fabber_nlls_run_hostmodel_host(C.byref(cfg), C.byref(nl), data.ctypes.data, C.byref(out), device, cb, None))
    finally:
        cfg.model = saved
    arrs["cost"] = arrs.pop("free_energy")
    return arrs


def postproc_host(holder, data, mvn, want=("mean", "var", "std", "zstat", "modelfit", "residuals", "noise_mean", "noise_std"),
                  device=0):
    cfg = holder.cfg
    V, T, P, N = cfg.n_voxels, cfg.n_times, cfg.n_params, holder.n_noise_outputs
    shapes = dict(mean=(P, V), var=(P, V), std=(P, V), zstat=(P, V), modelfit=(T, V), residuals=(T, V),
                  noise_mean=(N, V), noise_std=(N, V))
    data = _prepare_data(holder, data)
    mvn = np.ascontiguousarray(mvn, dtype=np.float64)
    pp = vbabi.FvbPostproc()
    arrs = {}
    for k in want:
        arrs[k] = np.full(shapes[k], np.nan)
        setattr(pp, k, arrs[k].ctypes.data)
    _check(lib().fabber_vb_postproc_host(C.byref(cfg), data.ctypes.data, mvn.ctypes.data, C.byref(pp), device))
    return arrs


def postproc_device(holder, data, mvn, want=("mean", "var", "std", "zstat", "modelfit", "residuals", "noise_mean", "noise_std"),
                    stream=None):
    """fabber_vb_postproc_device: the result images from device memory. data [T][V] (float32 or float64) and mvn
    [mvn_rows][V] (float64) are contiguous torch tensors on one device; the holder's design matrix, constants block and
    parameter table are uploaded next to them. Enqueued on `stream` (default: torch's current); returns the images as
    torch tensors on that device (read them after synchronising)."""
    import torch
    cfg = holder.cfg
    V, T, P, N = cfg.n_voxels, cfg.n_times, cfg.n_params, holder.n_noise_outputs
    assert data.is_cuda and data.is_contiguous() and data.dtype in (torch.float32, torch.float64) and tuple(data.shape) == (T, V)
    assert mvn.is_cuda and mvn.is_contiguous() and mvn.dtype == torch.float64 and tuple(mvn.shape) == (holder.n_mvn_rows, V)
    dev = data.device
    d = vbabi.FvbConfig.from_buffer_copy(cfg)
    d.data_f64 = 1 if data.dtype == torch.float64 else 0
    keep = []

    def up(arr):
        keep.append(torch.from_numpy(np.ascontiguousarray(arr)).to(dev))
        return keep[-1].data_ptr()
    if "design" in holder.keep:
        d.design = up(holder.keep["design"])
    if "constants" in holder.keep:
        d.model_consts = up(holder.keep["constants"])
    if "suppdata" in holder.keep:
        d.model_supp = up(holder.keep["suppdata"])
    if cfg.params_ext:  # (the table itself is device memory too; the result images read its transforms only)
        tab = holder.keep["param_table"][0]
        ext = vbabi.FvbParamTable()
        for f, a in tab.items():
            if f != "image_prior":
                setattr(ext, f, up(a))
        d.params_ext = up(np.frombuffer(bytes(ext), dtype=np.uint8))
    shapes = dict(mean=(P, V), var=(P, V), std=(P, V), zstat=(P, V), modelfit=(T, V), residuals=(T, V),
                  noise_mean=(N, V), noise_std=(N, V))
    pp = vbabi.FvbPostproc()
    out = {}
    for k in want:
        out[k] = torch.full(shapes[k], float("nan"), dtype=torch.float64, device=dev)
        setattr(pp, k, out[k].data_ptr())
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    _check(lib().fabber_vb_postproc_device(C.byref(d), data.data_ptr(), mvn.data_ptr(), C.byref(pp), C.c_void_p(stream.cuda_stream)))
    for t in keep:  # (the uploads are freed in the order of the stream the kernel reads them on)
        t.record_stream(stream)
    return out


def device_config(holder, dev, f64):
    """A copy of the holder's configuration whose pointer members are DEVICE memory on the torch device `dev` - design
    matrix, constants block, noise pattern, image priors, the parameter table with its images, init_mvn - for the entry
    points that take device pointers. f64: the element type of the series the call will be given. Returns (config, the
    tensors that hold the uploads): keep the second alive until the work that reads them is over."""
    import torch
    d = vbabi.FvbConfig.from_buffer_copy(holder.cfg)
    d.data_f64 = 1 if f64 else 0
    keep = []

    def up(arr):
        keep.append(torch.from_numpy(np.ascontiguousarray(arr)).to(dev))
        return keep[-1].data_ptr()
    for field, key in (("design", "design"), ("model_consts", "constants"), ("model_supp", "suppdata"), ("phi_index", "phi_index"),
                       ("init_mvn", "init_mvn")):
        if key in holder.keep:
            setattr(d, field, up(holder.keep[key]))
    images = {k: up(holder.keep["image_%d" % k]) for k in range(d.n_params) if "image_%d" % k in holder.keep}
    if d.params_ext:  # (the table itself is device memory too, and so is its list of image pointers)
        tab = holder.keep["param_table"][0]
        ext = vbabi.FvbParamTable()
        for f, a in tab.items():
            if f == "image_prior":
                a = np.array([images.get(k, 0) for k in range(d.n_params)], dtype=np.int64)  # (pointers; torch has no uint64)
            setattr(ext, f, up(a))
        d.params_ext = up(np.frombuffer(bytearray(bytes(ext)), dtype=np.uint8))
    else:
        for k, p in images.items():
            d.image_prior[k] = p
    return d, keep


def init_posterior_kernel_name(holder):
    """The kernel that writes the initial posterior of a configuration without init_mvn: "init<NAME>" (the kernel a model
    library compiled around its body's init_posterior, include/fabber_device_init_model.h), or "" - a built-in model, a
    library body without an init entry (a run without init_mvn answers -52), a given init_mvn, a refused configuration."""
    return lib().fabber_vb_init_posterior_kernel_name(C.byref(holder.cfg)).decode()


def init_posterior_host(holder, data, device=0):
    """fabber_vb_init_posterior_host: the initial posterior image [mvn_rows][V] of a library body with an init entry, from
    host arrays (-95 for a body without one and for a built-in model)."""
    data = _prepare_data(holder, data)
    img = np.full((holder.n_mvn_rows, holder.cfg.n_voxels), np.nan)
    _check(lib().fabber_vb_init_posterior_host(C.byref(holder.cfg), data.ctypes.data, img.ctypes.data, device))
    return img


def init_posterior_device(holder, data, stream=None):
    """fabber_vb_init_posterior_device: the same from device memory. data [T][V] (float32 or float64) is a contiguous torch
    tensor on a GPU; the holder's constants block, image priors and parameter table are uploaded next to it. Enqueued on
    `stream` (default: torch's current); returns the image as a torch tensor on that device (read it after
    synchronising)."""
    import torch
    cfg = holder.cfg
    V, T = cfg.n_voxels, cfg.n_times
    assert data.is_cuda and data.is_contiguous() and data.dtype in (torch.float32, torch.float64) and tuple(data.shape) == (T, V)
    d, keep = device_config(holder, data.device, data.dtype == torch.float64)
    img = torch.full((holder.n_mvn_rows, V), float("nan"), dtype=torch.float64, device=data.device)
    if stream is None:
        stream = torch.cuda.current_stream(data.device)
    _check(lib().fabber_vb_init_posterior_device(C.byref(d), data.data_ptr(), img.data_ptr(), C.c_void_p(stream.cuda_stream)))
    for t in keep:  # (the uploads are freed in the order of the stream the kernel reads them on)
        t.record_stream(stream)
    return img


def convergence_trace(conv, F, max_iterations=10, max_trials=10, min_fchange=0.01, stop_at_done=True):
    F = np.ascontiguousarray(F, dtype=np.float64)
    n = len(F)
    done = np.zeros(n, dtype=np.int32)
    save = np.zeros(n, dtype=np.int32)
    revert = np.zeros(n, dtype=np.int32)
    alpha = np.zeros(n)
    conv = vbabi.CONV_NAMES[conv] if isinstance(conv, str) else conv
    m = lib().fabber_vb_convergence_trace(conv, max_iterations, max_trials, min_fchange, F.ctypes.data, n,
                                          done.ctypes.data, save.ctypes.data, revert.ctypes.data, alpha.ctypes.data,
                                          int(stop_at_done))
    return done[:m].astype(bool), save[:m].astype(bool), revert[:m].astype(bool), alpha[:m]


def device_math(what, values):
    """Building blocks of vb_math.h evaluated on the device (fabber_vb_device_math): what = "exp_acc" | "exp" on a
    vector, or "invert4" on packed 4 x 4 symmetric matrices [n][10] -> (packed inverses [n][10], log|det| [n])."""
    L = lib()
    L.fabber_vb_device_math.restype = C.c_int32
    L.fabber_vb_device_math.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    x = np.ascontiguousarray(values, dtype=np.float64)
    code = {"exp_acc": 0, "exp": 1, "invert4": 2}[what]
    n = x.shape[0]
    out = np.empty((n, 11) if code == 2 else n)
    _check(L.fabber_vb_device_math(code, n, x.ctypes.data, out.ctypes.data))
    return (out[:, :10], out[:, 10]) if code == 2 else out


def ldl_inverse(a):
    """Host twin of the in-register LDL^T inverse; a: symmetric PxP. Returns (inv, logabs, sign, ok)."""
    a = np.asarray(a, dtype=np.float64)
    P = a.shape[0]
    packed = np.array([a[i, j] for i in range(P) for j in range(i + 1)])
    inv = np.zeros_like(packed)
    logabs = C.c_double()
    sign = C.c_int32()
    rc = lib().fabber_vb_ldl_inverse(P, packed.ctypes.data, inv.ctypes.data, C.byref(logabs), C.byref(sign))
    out = np.zeros((P, P))
    k = 0
    for i in range(P):
        for j in range(i + 1):
            out[i, j] = out[j, i] = inv[k]
            k += 1
    return out, logabs.value, sign.value, rc == 0


# ---- spatial VB --------------------------------------------------------------------------------
PROGRESS_CB = C.CFUNCTYPE(None, C.c_int, C.c_int)


def run_spatial_host(holder, spatial, data, device=0, progress_cb=None, devices=None):
    """Spatial VB on the GPU from host arrays. spatial: vbabi.SpatialHolder. devices: "all" or a list of device
    indices - z-slabs of the one volume on several devices, driven by this process
    (fabber_vb_run_spatial_host_multi)."""
    cfg = holder.cfg
    data = _prepare_data(holder, data)
    V = cfg.n_voxels
    arrs = dict(
        mvn=np.full((holder.n_mvn_rows, V), np.nan),
        free_energy=np.full(V, np.nan),
        status=np.full(V, -1, dtype=np.int32),
        iterations=np.full(V, -1, dtype=np.int32),
    )
    out = vbabi.FvbOutputs()
    for k, a in arrs.items():
        setattr(out, k, a.ctypes.data)
    L = lib()
    L.fabber_vb_run_spatial_host.restype = C.c_int32
    L.fabber_vb_run_spatial_host.argtypes = [C.POINTER(vbabi.FvbConfig), C.POINTER(vbabi.FvbSpatial), C.c_void_p,
                                             C.POINTER(vbabi.FvbOutputs), C.c_int32, C.c_void_p]
    cb = PROGRESS_CB(progress_cb) if progress_cb else None
    if devices is not None:
        L.fabber_vb_run_spatial_host_multi.restype = C.c_int32
        L.fabber_vb_run_spatial_host_multi.argtypes = [C.POINTER(vbabi.FvbConfig), C.POINTER(vbabi.FvbSpatial), C.c_void_p,
                                                       C.POINTER(vbabi.FvbOutputs), C.c_void_p, C.c_int32, C.c_void_p]
        ids = None if devices == "all" else (C.c_int32 * len(devices))(*devices)
        _check(L.fabber_vb_run_spatial_host_multi(C.byref(cfg), C.byref(spatial.sp), data.ctypes.data, C.byref(out), ids,
                                                  0 if ids is None else len(devices), C.cast(cb, C.c_void_p) if cb else None))
    else:
        _check(L.fabber_vb_run_spatial_host(C.byref(cfg), C.byref(spatial.sp), data.ctypes.data, C.byref(out), device,
                                            C.cast(cb, C.c_void_p) if cb else None))
    arrs["setup_failed"] = (arrs["status"] & 0x100) != 0
    arrs["status"] = arrs["status"] & 0xFF
    return arrs


def initial_mvn(holder, data):
    """The initial posterior image [mvn_rows][V] of a holder, as Vb::BuildInitialMvn writes it for the routes that
    evaluate the model on the host: the model's initial posterior in Fabber space (means from post_mean or the image
    prior, variances from post_var, no covariances) and the noise posterior as its mean and variance. The exponential
    model's InitVoxelPosterior sets amplitude i to max(y) / (num-exps + i) (examples/fwdmodel_exp.cc). White noise."""
    cfg = holder.cfg
    V, T, P = cfg.n_voxels, cfg.n_times, cfg.n_params
    assert not cfg.params_ext and cfg.noise == vbabi.NOISE_WHITE
    n = P + cfg.n_phis
    nCov = n * (n + 1) // 2
    img = np.zeros((vbabi.mvn_rows(n), V))
    data_max = np.asarray(data, dtype=np.float64).max(axis=0) if cfg.model == vbabi.MODEL_EXP else None
    for i in range(P):
        tr = cfg.transform[i]
        if cfg.prior_type[i] == vbabi.PRIOR_IMAGE:
            mean = np.array(holder.keep["image_%d" % i], dtype=np.float64)
        else:
            mean = np.full(V, cfg.post_mean[i])
        if data_max is not None and i % 2 == 0:
            mean = data_max / (P // 2 + i // 2)
        img[nCov + i] = [vbabi.to_fabber(tr, float(m)) for m in mean]
        img[i * (i + 1) // 2 + i] = vbabi.to_fabber_var(tr, cfg.post_var[i])
    for k in range(cfg.n_phis):
        b, c = cfg.noise_post_b[k], cfg.noise_post_c[k]
        q = P + k
        img[q * (q + 1) // 2 + q] = b * b * c  # GammaDist variance / mean, as OutputAsMVN
        img[nCov + q] = b * c
    img[-1] = 1.0
    return img


def jacobian_callback(linearise, T, P):
    """fvb_linearise_fn from a Python function that returns the linearisation itself: linearise(params [n][P] Fabber
    space, voxel ids [n]) -> (g [n][T], J [n][T][P]) - a linear model hands over its design matrix exactly. Keep the
    returned object alive for the duration of the call."""
    def cb(user, n, ids, means, lin):
        try:
            v = np.ctypeslib.as_array(ids, (n,))
            m = np.ctypeslib.as_array(means, (n * P,)).reshape(n, P)
            out = np.ctypeslib.as_array(lin, (n * T * (P + 1),)).reshape(n, T * (P + 1))
            g, J = linearise(m.copy(), v.copy())
            out[:, :T] = np.broadcast_to(np.asarray(g, dtype=np.float64), (n, T))
            out[:, T:] = np.broadcast_to(np.asarray(J, dtype=np.float64), (n, T, P)).reshape(n, -1)
            return 0
        except Exception:  # noqa: BLE001 (the engine reports -54)
            return 1
    return LINEARISE_FN(cb)


def run_spatial_hostmodel_host(holder, spatial, data, linearise, device=0, progress_cb=None):
    """Spatial VB with the model evaluated by the caller (fabber_vb_run_spatial_hostmodel_host): up to 8 parameters one
    voxel per lane, 9 to 32 one wavefront per voxel (white noise with one precision). `linearise` is either what
    recentre_callback(model, T, P) returns (the reference's central differences about the current means) or a Python
    function for jacobian_callback (g and J directly). The initial posterior is the holder's init_mvn if it has one,
    else initial_mvn(holder, data). The holder's model fields are not read. Returns the dict of run_spatial_host."""
    cfg = holder.cfg
    data = _prepare_data(holder, data)
    V, T, P = cfg.n_voxels, cfg.n_times, cfg.n_params
    cb = linearise if isinstance(linearise, LINEARISE_FN) else jacobian_callback(linearise, T, P)
    init = None if cfg.init_mvn else np.ascontiguousarray(initial_mvn(holder, data))
    arrs = dict(
        mvn=np.full((holder.n_mvn_rows, V), np.nan),
        free_energy=np.full(V, np.nan),
        status=np.full(V, -1, dtype=np.int32),
        iterations=np.full(V, -1, dtype=np.int32),
    )
    out = vbabi.FvbOutputs()
    for k, a in arrs.items():
        setattr(out, k, a.ctypes.data)
    L = lib()
    L.fabber_vb_run_spatial_hostmodel_host.restype = C.c_int32
    L.fabber_vb_run_spatial_hostmodel_host.argtypes = [C.POINTER(vbabi.FvbConfig), C.POINTER(vbabi.FvbSpatial), C.c_void_p,
                                                       C.POINTER(vbabi.FvbOutputs), C.c_int32, LINEARISE_FN, C.c_void_p,
                                                       C.c_void_p]
    pcb = PROGRESS_CB(progress_cb) if progress_cb else None
    saved = (cfg.model, cfg.design, cfg.init_mvn)
    cfg.model, cfg.design = vbabi.MODEL_HOSTJAC, None
    if init is not None:
        cfg.init_mvn = init.ctypes.data
    try:
        _check(L.fabber_vb_run_spatial_hostmodel_host(C.byref(cfg), C.byref(spatial.sp), data.ctypes.data, C.byref(out), device,
                                                      cb, None, C.cast(pcb, C.c_void_p) if pcb else None))
    finally:
        cfg.model, cfg.design, cfg.init_mvn = saved
    arrs["setup_failed"] = (arrs["status"] & 0x100) != 0
    arrs["status"] = arrs["status"] & 0xFF
    return arrs


class SpatialMultiRun:
    """One spatial VB problem resident on several devices (fabber_vb_spatial_multi_*): open uploads, run() is one
    complete run on the resident data (may be repeated), results() downloads, close() frees."""

    def __init__(self, holder, spatial, data, devices, want=("free_energy", "status", "iterations")):
        self.holder, self.spatial = holder, spatial
        cfg = holder.cfg
        self._data = _prepare_data(holder, data)
        V = cfg.n_voxels
        self.arrs = dict(mvn=np.full((holder.n_mvn_rows, V), np.nan))
        if "free_energy" in want:
            self.arrs["free_energy"] = np.full(V, np.nan)
        if "status" in want:
            self.arrs["status"] = np.full(V, -1, dtype=np.int32)
        if "iterations" in want:
            self.arrs["iterations"] = np.full(V, -1, dtype=np.int32)
        self.out = vbabi.FvbOutputs()
        for k, a in self.arrs.items():
            setattr(self.out, k, a.ctypes.data)
        L = self.L = lib()
        L.fabber_vb_spatial_multi_open.restype = C.c_int32
        L.fabber_vb_spatial_multi_open.argtypes = [C.POINTER(vbabi.FvbConfig), C.POINTER(vbabi.FvbSpatial), C.c_void_p,
                                                   C.POINTER(vbabi.FvbOutputs), C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
        for name in ("fabber_vb_spatial_multi_run", "fabber_vb_spatial_multi_results"):
            getattr(L, name).restype = C.c_int32
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p]
        L.fabber_vb_spatial_multi_slabs.restype = C.c_int32
        L.fabber_vb_spatial_multi_slabs.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_char_p, C.c_int32]
        L.fabber_vb_spatial_multi_close.restype = C.c_int32
        L.fabber_vb_spatial_multi_close.argtypes = [C.c_void_p]
        ids = None if devices == "all" else (C.c_int32 * len(devices))(*devices)
        self.h = C.c_void_p()
        _check(L.fabber_vb_spatial_multi_open(C.byref(cfg), C.byref(spatial.sp), self._data.ctypes.data, C.byref(self.out), ids,
                                              0 if ids is None else len(devices), C.byref(self.h)))

    def run(self):
        _check(self.L.fabber_vb_spatial_multi_run(self.h, None))

    def slabs(self):
        n = C.c_int32(0)
        buf = C.create_string_buffer(64)
        _check(self.L.fabber_vb_spatial_multi_slabs(self.h, C.byref(n), buf, 64))
        return n.value, buf.value.decode()

    def results(self):
        _check(self.L.fabber_vb_spatial_multi_results(self.h, C.byref(self.out)))
        r = dict(self.arrs)
        if "status" in r:
            r["setup_failed"] = (r["status"] & 0x100) != 0
            r["status"] = r["status"] & 0xFF
        return r

    def close(self):
        if self.h:
            self.L.fabber_vb_spatial_multi_close(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def test_unlink_slab_pair(pair):
    """Fault injection for tests (fabber_vb_test_unlink_slab_pair): the next multi-device spatial run of this thread
    leaves the slab above `pair` without its inboxes' writer."""
    L = lib()
    L.fabber_vb_test_unlink_slab_pair.restype = None
    L.fabber_vb_test_unlink_slab_pair.argtypes = [C.c_int32]
    L.fabber_vb_test_unlink_slab_pair(pair)


def neighbours(coords, spatial_dims=3):
    """First-neighbour table of the spatial driver (host code, no GPU): [V][6], -1 = none."""
    coords = np.ascontiguousarray(coords, dtype=np.int32)
    V = coords.shape[1]
    nn = np.full((V, 6), -1, dtype=np.int32)
    L = lib()
    L.fabber_vb_neighbours.restype = C.c_int32
    L.fabber_vb_neighbours.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    _check(L.fabber_vb_neighbours(coords.ctypes.data, V, spatial_dims, nn.ctypes.data))
    return nn
