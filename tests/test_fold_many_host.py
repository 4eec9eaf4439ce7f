"""dspsr_amd_fold_fold_many without a GPU: the kernel's code objects use no scratch, the header and the ctypes binding agree, the
argument checks that need no device, the tool's repeated -P / -c, and the multi-pulsar refusals of LoadToFold.  CPU only."""
import ctypes as C
import importlib.util
import json
import os
import re
import subprocess

import pytest

from test_kernel_resources import LIB, _code_objects, _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fold_many_kernels_use_no_scratch():
    ks = {}
    for co in _code_objects(open(LIB, "rb").read()):
        ks.update(_kernels(co))
    names = sorted(ks)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    many = {d.split("(")[0].replace("void dspsr_amd::", ""): ks[n] for d, n in zip(dem, names) if "k_fold_many<" in d}
    assert sorted(many) == ["k_fold_many<1, 1>", "k_fold_many<1, 4>", "k_fold_many<2, 1>", "k_fold_many<2, 2>", "k_fold_many<4, 1>"]
    for name, kd in many.items():
        assert kd[".private_segment_fixed_size"] == 0, name
        assert kd[".group_segment_fixed_size"] + 2048 * 4 * 4 <= 160 * 1024, name     # descriptors + the largest chunk image


def test_header_declares_fold_many_and_the_binding_matches():
    from dspsr_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dspsr_amd.h")).read(), flags=re.S)
    m = re.search(r"int\s+dspsr_amd_fold_fold_many\s*\(([^)]*)\)\s*;", text)
    assert m, "dspsr_amd_fold_fold_many is not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["dspsr_amd_fold* const* folds", "uint32_t nfold", "const float* in_dev", "uint64_t in_chan_stride",
                    "uint64_t in_pol_stride", "uint32_t* nshared"]
    res, argtypes = _lib.SYMBOLS["dspsr_amd_fold_fold_many"]
    assert res is C.c_int
    assert argtypes == [C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32)]
    assert int(re.search(r"#define\s+DSPSR_AMD_FOLD_MANY_MAX\s+(\d+)", text).group(1)) == 8


def test_fold_many_argument_checks_without_a_device():
    from dspsr_amd import _lib
    n = C.c_uint32(7)
    assert _lib.lib.dspsr_amd_fold_fold_many(None, 0, None, 0, 0, C.byref(n)) == _lib.OK and n.value == 0
    assert _lib.lib.dspsr_amd_fold_fold_many(None, 1, C.c_void_p(4096), 0, 0, None) == _lib.EINVAL
    arr = (C.c_void_p * 2)(None, None)
    assert _lib.lib.dspsr_amd_fold_fold_many(arr, 2, C.c_void_p(4096), 0, 0, None) == _lib.EINVAL
    assert _lib.lib.dspsr_amd_fold_fold_many(arr, 2, None, 0, 0, None) == _lib.EINVAL


def _tool():
    spec = importlib.util.spec_from_file_location("dspsr_amd_fold_tool", os.path.join(ROOT, "tools", "dspsr_amd_fold.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_repeated_pulsars_parse_into_targets(tmp_path):
    tool = _tool()
    pc = tmp_path / "vela.polyco"
    pc.write_text(json.load(open(os.path.join(ROOT, "tests", "golden", "vela_polyco.json")))["text"])
    a = tool.parse_args(["-F", "16:D", "-P", str(pc), "-c", "0.004", "-c", "0.0005", "x.dada"])
    ts = tool.fold_targets(a, 0, 1e6, 55299, 7545.0)
    assert [t.name for t in ts] == ["vela.polyco", "P=0.004", "P=0.0005"]
    assert ts[0].polyco is not None and ts[0].nbin == 1024
    assert [(t.folding_period, t.nbin) for t in ts[1:]] == [(0.004, 1024), (0.0005, 256)]
    a = tool.parse_args(["-F", "16:D", "-b", "64", "-c", "0.004", "-c", "0.002", "x.dada"])
    assert [t.nbin for t in tool.fold_targets(a, a.nbin, 1e6, 55299, 7545.0)] == [64, 64]
    for one in (["-c", "0.004"], ["-P", str(pc)], ["-P", str(pc), "-c", "0.004"]):   # today's single pulsar
        a = tool.parse_args(["-F", "16:D"] + one + ["x.dada"])
        assert tool.fold_targets(a, 0, 1e6, 55299, 7545.0) == []


def test_several_targets_refuse_the_multi_gpu_exchange():
    from dspsr_amd import DspsrAmdError, pipeline
    cfg = pipeline.Config(nchan=16, dispersion_measure=30.0, nbin=64, ndim=4)
    info = pipeline.InputInfo(centre_frequency=1382.0, bandwidth=-16.0, nchan=2, tsamp_us=1.0 / 32.0)
    targets = [pipeline.FoldTarget("a", folding_period=0.004), pipeline.FoldTarget("b", folding_period=0.002)]
    with pytest.raises(DspsrAmdError, match="sub-band"):
        pipeline.LoadToFold(cfg, info, subband=0, targets=targets)
    lt = pipeline.LoadToFold.__new__(pipeline.LoadToFold)        # the communicator setters refuse before touching a device
    lt.pulsars = [object(), object()]
    with pytest.raises(DspsrAmdError, match="one pulsar"):
        lt.set_communicator(None, 0, 2)
    with pytest.raises(DspsrAmdError, match="one pulsar"):
        lt.set_rccl_communicator(object())
