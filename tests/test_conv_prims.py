"""The hand-placed primitives of the 16-bit forward conv kernels have ONE home.  No GPU, no compiler: source text only.

The sources of the forward trunk (H16SRCS in csrc/Makefile) are built from a handful of inline-asm forms -- the counted waits, the
uncounted LDS read, the MFMA with its accumulator tied in place, the packed conversion and the packed ReLU.  Each used to be copied
into nearly every file, and a fix had to find every copy.  They now live in csrc/conv_prims.inc (and, the two packed forms, in
csrc/ap_common.h); this test keeps the copies from growing back:

  * each asm string appears in the tree at most as often as the header documents forms of it (FORMS below: e.g. the vmcnt wait
    with and without a scheduling fence, the in-place MFMA on a "+v" and on a "+a" accumulator), and at least once;
  * none of them appears in any .hip file;
  * the Makefile's HDRS names every .inc an H16SRCS source includes, so that editing the header rebuilds them.

A bare `s_waitcnt vmcnt(0)` (stem.hip) is not the templated form `vmcnt(%0)` and is not counted.
"""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "airpose_amd", "csrc")

# asm string -> (documented forms, where they live)
FORMS = {
    '"s_waitcnt vmcnt(%0)"': (2, "conv_prims.inc"),             # ap_wait_vm (fenced), ap_wait_vm_bare
    '"s_waitcnt lgkmcnt(%0)"': (1, "conv_prims.inc"),           # ap_wait_lgkm
    '"ds_read_b128 %0, %1 offset:%2"': (2, "conv_prims.inc"),   # ap_lds_read (return value), ap_lds_read_to (out parameter)
    'AP_MFMA16_ASM " %0, %1, %2, %0"': (2, "conv_prims.inc"),   # ap_mfma_acc_v, ap_mfma_acc_a
    '"v_pk_max_i16 %0, %1, 0"': (1, "ap_common.h"),             # ap_relu_pk
    'AP_CVTPK_ASM " %0': (1, "ap_common.h"),                    # pack_bf16x2
}


def _texts():
    paths = sorted(p for ext in ("*.hip", "*.inc", "*.h") for p in glob.glob(os.path.join(CSRC, ext)))
    assert len(paths) > 40, "the kernel sources were not found"
    return {os.path.basename(p): open(p).read() for p in paths}


def _make_var(text, name):
    return re.search(r"^%s\s*=\s*(.*)$" % name, text, re.M).group(1).split()


def test_each_shared_asm_form_is_defined_once():
    texts = _texts()
    for s, (forms, home) in FORMS.items():
        where = {name: t.count(s) for name, t in texts.items() if s in t}
        assert where == {home: forms}, "%s: expected %d in %s only, found %r" % (s, forms, home, where)
        assert not any(name.endswith(".hip") for name in where), s


def test_hdrs_names_every_include_of_the_h16_sources():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    h16, hdrs = _make_var(mk, "H16SRCS"), set(_make_var(mk, "HDRS"))
    assert "conv_prims.inc" in hdrs and not os.path.exists(os.path.join(CSRC, "bi_helpers.inc"))
    used = set()
    for src in h16:
        incs = set(re.findall(r'^\s*#include\s+"([^"]+\.inc)"', open(os.path.join(CSRC, src)).read(), re.M))
        assert incs <= hdrs, "%s includes %s, which HDRS does not name" % (src, sorted(incs - hdrs))
        used |= incs
    assert "conv_prims.inc" in used
