"""CPU: the product library loads and exports every symbol include/pymes_amd.h declares
(no compute calls: there is no GPU here)."""
import os
import re

from pymes_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_are_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "pymes_amd.h")).read()
    declared = set(re.findall(r"\b(pymes_[a-zA-Z0-9_]+)\s*\(", text))
    assert declared, "no declarations found"
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    lib = _lib.Library()                      # libpymes_amd.so (HIP); raises if missing
    assert lib.backend == "hip-gfx950"
    for name in declared:
        assert hasattr(lib.dll, name), name


def test_missing_library_fails_loudly(tmp_path):
    import pytest
    with pytest.raises(_lib.PymesError, match="no CPU fallback"):
        _lib.Library(str(tmp_path / "nope.so"))


def test_library_override(tmp_path):
    """PYMES_AMD_LIBRARY=<path>: the loader takes that build (a missing one fails loudly; the backend check still applies).
    In a process of its own: the variable is read when the module is imported."""
    import subprocess
    import sys
    code = ("from pymes_amd import _lib\n"
            "assert _lib.DEFAULT_PATH.endswith('other_build.so'), _lib.DEFAULT_PATH\n"
            "try:\n    _lib.Library()\nexcept _lib.PymesError as e:\n    assert 'no CPU fallback' in str(e); print('refused')\n")
    env = dict(os.environ, PYMES_AMD_LIBRARY=str(tmp_path / "other_build.so"), PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "refused" in out.stdout, out.stderr


def test_unrecorded_stream_work_goes_through_the_ordered_layer():
    """kernels.hip defers launches in the phase queue; whatever is not recorded there, in any HIP unit, must launch the queue
    first.  The ten runtime calls that do so are poisoned below their wrappers in launch.h (the compiler refuses a bypass in
    every unit that includes it); a raw kernel launch cannot be poisoned, so it is looked for here, over launch.h and every
    unit together: only phase_flush (the flush itself) and try_launch_kernel may hold one, nothing above the poison but the
    wrappers may name a poisoned call, and no unit names one at all."""
    csrc = os.path.join(ROOT, "pymes_amd", "csrc")

    def read(name):
        return re.sub(r"//[^\n]*|/\*.*?\*/", "", open(os.path.join(csrc, name)).read(), flags=re.S)

    units = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    assert "kernels.hip" in units
    others = units + sorted(f for f in os.listdir(csrc) if f.endswith(".h") and f != "launch.h")
    srcs = {f: read(f) for f in ["launch.h"] + others}
    for f, src in srcs.items():
        assert not re.search(r"#\s*define\s+hip", src), f
    layer = srcs["launch.h"]
    poisoned = re.findall(r"#pragma GCC poison ([^\n]+)", layer)
    names = " ".join(poisoned).split()
    assert sorted(names) == sorted(["hipMemcpyAsync", "hipMemsetAsync", "hipMemcpy", "hipStreamSynchronize", "hipEventRecord",
                                    "hipStreamWaitEvent", "hipGraphLaunch", "hipStreamBeginCapture", "hipStreamEndCapture",
                                    "hipFree"])
    above = layer[:layer.index("#pragma GCC poison")]
    for name in names:
        assert len(re.findall(r"\b%s\b" % name, above)) == 1, name         # its wrapper
        for f in others:
            assert not re.search(r"\b%s\b" % name, srcs[f]), (f, name)
            assert "#pragma GCC poison" not in srcs[f], f
    # every unit is under the poison before it defines anything
    for f in units:
        inc = re.search(r'#include "launch\.h"', srcs[f])
        body = re.search(r"\{", srcs[f])
        assert inc and body and inc.start() < body.start(), f
    # raw launches: split each file at the top-level function headers that may hold one
    raw = r"hipLaunchKernelGGL|<<<|hipLaunchKernel\b|hipModuleLaunchKernel|hipExtLaunchKernel"
    owners = []
    for f, src in srcs.items():
        for m in re.finditer(raw, src):
            head = src[:m.start()]
            found = re.findall(r"\n(?:void|hipError_t) (\w+)\([^;{]*\) \{\n", head)
            assert found and found[-1] in ("phase_flush", "try_launch_kernel"), (f, found[-1:], src[m.start():m.start() + 80])
            owners.append((f, found[-1]))
    assert sorted(owners) == [("kernels.hip", "phase_flush"), ("kernels.hip", "phase_flush"), ("launch.h", "try_launch_kernel")]
