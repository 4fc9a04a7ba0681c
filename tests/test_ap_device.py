"""What a launcher caches per device has ONE home, csrc/ap_device.h.  No GPU.

hipFuncSetAttribute and the CU count are per device, so the launch side keys its caches by the current device id.  Every launcher
used to write that rule out by hand -- a static array, the device query, the opt-in block, the error returns -- and the copies had
drifted (fitting.hip: a process-wide flag; six CU-count caches with three conventions; plain bools under handles that other threads
may use).  They now call ap_device / ap_once_per_device / ap_lds_optin.  Two kinds of test:

  * source text only, in the style of test_conv_prims.py: the copies must not grow back;
  * tests/host/ap_device_once.cpp, a stand-alone host program (its own main, no HIP call) that races 8 threads through every slot
    of the once-flag, built with the project's compiler under ThreadSanitizer and run here.  Where ThreadSanitizer cannot be linked
    or cannot start on the build machine, the same program is built and run without it, and the test says so in its output.
"""
import glob
import os
import re
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "airpose_amd", "csrc")
HOME = "ap_device.h"


def _texts():
    paths = sorted(p for ext in ("*.hip", "*.inc", "*.h") for p in glob.glob(os.path.join(CSRC, ext)))
    assert len(paths) > 40, "the kernel sources were not found"
    return {os.path.basename(p): open(p).read() for p in paths}


def test_the_runtime_calls_are_named_in_the_header_only():
    texts = _texts()
    for word in ("hipFuncSetAttribute", "hipDeviceAttributeMultiprocessorCount"):
        assert {name for name, t in texts.items() if word in t} == {HOME}, word
    assert not [name for name, t in texts.items() if "ap_current_device" in t]


def test_no_source_keeps_a_per_device_array_or_a_process_wide_flag():
    for name, t in _texts().items():
        if name.endswith(".hip"):
            assert not re.search(r"\[\s*AP_MAX_DEVICES\s*\]", t), "%s declares a per-device array of its own" % name
        # `static const hipError_t attr = hipFuncSetAttribute(...)`: once per process, on whichever device came first, failure cached
        assert not re.search(r"static\s+const\s+hipError_t\s+\w+\s*=\s*hip", t), "%s caches a runtime call's result for the process" % name


def test_hdrs_names_the_header_and_the_launchers_see_it():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert HOME in re.search(r"^HDRS\s*=\s*(.*)$", mk, re.M).group(1).split()
    assert re.search(r'^\s*#include\s+"%s"' % re.escape(HOME), open(os.path.join(CSRC, "kernels.h")).read(), re.M)


def test_once_per_device_under_thread_sanitizer(tmp_path):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1)
    assert shutil.which(hipcc), "%s: the test needs the compiler the build uses" % hipcc
    src = os.path.join(REPO, "tests", "host", "ap_device_once.cpp")

    def build_and_run(name, extra):
        exe = str(tmp_path / name)
        c = subprocess.run([hipcc, "-std=c++17", "-O1", "-g", "-pthread"] + extra + [src, "-o", exe], capture_output=True, text=True)
        if c.returncode:
            return None, c.stderr
        return subprocess.run([exe], capture_output=True, text=True, timeout=300), ""

    r, why = build_and_run("once_tsan", ["-Xarch_host", "-fsanitize=thread"])
    if r is not None and "FATAL: ThreadSanitizer" in r.stderr:           # linked, but its runtime cannot start here (address-space layout)
        r, why = None, r.stderr
    if r is None:
        print("ThreadSanitizer is not usable on this machine, running the program UNSANITISED:\n" + why[-600:])
        r, why = build_and_run("once_plain", [])
        assert r is not None, why
    else:
        print("built and run under ThreadSanitizer")
    print(r.stdout + r.stderr)
    assert r.returncode == 0 and "ThreadSanitizer" not in r.stderr and " 0 errors" in r.stdout
