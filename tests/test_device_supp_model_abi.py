"""The ABI of per-voxel supplementary data for a model library's device body, as far as it can be checked without a GPU:
fvb_config's two new fields (model_supp, n_model_supp) in include/fabber_vb.h and in their ctypes mirror, the version
both state, and vbabi.build_config(suppdata=...)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fabber_core_amd import vbabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = [dict(name="amp", prior=(1.0, 1e6), post=(1.0, 1e6), prior_type="N", transform=vbabi.TRANSFORM_IDENTITY),
          dict(name="r", prior=(1.0, 100.0), post=(1.0, 1.5), prior_type="N", transform=vbabi.TRANSFORM_LOG)]


def header():
    with open(os.path.join(ROOT, "include", "fabber_vb.h")) as fh:
        return fh.read()


def config(V, T, **kw):
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model="suppconv", dt=0.25, params=PARAMS, **kw)


def test_abi_version_is_11_in_the_header_and_in_its_mirror():
    m = re.search(r"^#define\s+FVB_ABI_VERSION\s+(\d+)", header(), re.M)
    assert m and int(m.group(1)) == 11
    assert vbabi.FVB_ABI_VERSION == 11
    assert config(3, 4).cfg.abi_version == 11


def test_the_two_fields_end_the_configuration_in_the_header_and_in_its_mirror():
    body = re.search(r"typedef struct fvb_config\s*\{(.*?)\}\s*fvb_config;", header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [d.strip() for d in body.split(";") if d.strip()]
    assert re.fullmatch(r"const double \*model_supp", members[-2]) and re.fullmatch(r"int32_t n_model_supp", members[-1])
    assert re.fullmatch(r"int32_t n_model_consts", members[-3])
    names = [f[0] for f in vbabi.FvbConfig._fields_]
    assert names[-3:] == ["n_model_consts", "model_supp", "n_model_supp"]
    assert vbabi.FvbConfig._fields_[-2][1] is C.c_void_p and vbabi.FvbConfig._fields_[-1][1] is C.c_int32


def test_size_is_the_parents_plus_a_pointer_and_a_padded_count():
    class Parent(C.Structure):
        _fields_ = vbabi.FvbConfig._fields_[:-2]
    assert C.sizeof(Parent) % 8 == 0  # (n_model_consts was followed by four bytes of padding already)
    assert C.sizeof(vbabi.FvbConfig) == C.sizeof(Parent) + 8 + 8
    assert vbabi.FvbConfig.model_supp.offset == C.sizeof(Parent)
    assert vbabi.FvbConfig.n_model_supp.offset == C.sizeof(Parent) + 8


def test_build_config_sets_both_fields_and_keeps_the_array():
    V, T = 5, 4
    supp = np.arange(T * V, dtype=np.float32).reshape(T, V)[:, ::-1]  # (neither float64 nor contiguous: a copy is kept)
    h = config(V, T, suppdata=supp)
    kept = h.keep["suppdata"]
    assert kept.dtype == np.float64 and kept.flags["C_CONTIGUOUS"] and np.array_equal(kept, supp)
    assert h.cfg.model_supp == kept.ctypes.data and h.cfg.n_model_supp == T
    more = config(V, T, suppdata=np.zeros((T + 3, V)))  # (more rows than timepoints are the model's business)
    assert more.cfg.n_model_supp == T + 3
    none = config(V, T)
    assert not none.cfg.model_supp and none.cfg.n_model_supp == 0 and "suppdata" not in none.keep


@pytest.mark.parametrize("shape", [(4,), (4, 6), (5, 4), (4, 5, 1)])
def test_build_config_rejects_a_wrong_shape(shape):
    with pytest.raises(ValueError, match="suppdata"):
        config(5, 4, suppdata=np.zeros(shape))
