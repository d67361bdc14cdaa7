"""A default build of libplhip.so carries no timing instrumentation: no clock reads (s_memtime / s_memrealtime), no s_sleep
and no timeline stamp buffers in any device object, and the fused 14 x 14 kernel is instantiated only in the forms its
launcher reaches.  Reads the ISA the build keeps beside the objects (csrc/*-gfx950.s); a `make EXPERIMENTS=1` build has the
stamps on purpose and fails here."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "paddle-lite_amd", "csrc")


def _isa():
    files = sorted(glob.glob(os.path.join(CSRC, "*-gfx950.s")))
    srcs = sorted(glob.glob(os.path.join(CSRC, "*.hip")))
    assert len(files) == len(srcs), "build the library first (one kept ISA file per translation unit)"
    return {os.path.basename(f): open(f).read() for f in files}


def test_default_build_has_no_clock_reads_sleeps_or_stamp_buffers():
    bad = []
    for name, text in _isa().items():
        for ins in ("s_memtime", "s_memrealtime", "s_sleep"):
            if re.search(r"^\s*%s\b" % ins, text, re.M):
                bad.append("%s: %s" % (name, ins))
        for sym in set(re.findall(r"\b\w*stamps\w*\b", text)):
            bad.append("%s: symbol %s" % (name, sym))
    assert not bad, bad


def test_fused_14x14_kernel_has_only_reachable_instantiations():
    # launch_fused_t: 2 tile heights (MTW) x (int8 out: 4 activation pairs; int32 / fp32 out: 2)
    text = _isa()["fused_dwpw_i8-hip-amdgcn-amd-amdhsa-gfx950.s"]
    kernels = set(re.findall(r"^(_Z\w*fused_dwpw14_kernel\w*):", text, re.M))
    assert len(kernels) == 16, sorted(kernels)
