"""The argument heads of the kernels launched per PCG iteration or per Gauss-Newton step (csrc/tsgo_kernels.h, "Argument heads"), read off
the built libraries' gfx950 code (tools/kernarg_heads.py; no GPU): in libtsgo_hip.so every instantiation has arguments preloaded into
SGPRs and waits for no scalar load from the kernarg segment before its first vector memory load; libtsgo_hip_plain.so, the same
sources without the build's preload option, has no preloaded argument anywhere — the check can tell the two apart."""
import importlib.util
import os
import re

import pytest

from toyslam_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("kernarg_heads", os.path.join(ROOT, "tools", "kernarg_heads.py"))
kh = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kh)

# Kernels that cannot meet the rule, by base name (at most three), the instantiations meant, and why.
#   k_bcsr_residual with 64 lanes per row as a smoothing sweep or power-iteration step (MODE 1, 2): the row is wave-uniform, so its
#   bounds AND its epilogue operands (right-hand side, own entry, diagonal inverse) come through the scalar cache before any vector
#   load is issued; with n, xcd8, st, ptr, col, the matrix and the gathered vector that is two ints and seven pointers, 16 dwords:
#   the diagonal inverse's pointer is fetched from the kernarg segment.  Every other instantiation of the kernel is held to the rule.
EXEMPT = {"k_bcsr_residual": re.compile(r"k_bcsr_residualI[df]Li64ELi[12]E")}
assert len(EXEMPT) <= 3


def _built(path):
    """The library as it was built (__graft_entry__.build(), or python -m toyslam_amd.build): read, never compiled here."""
    if not os.path.exists(path):
        pytest.fail("%s is missing: run __graft_entry__.build() or python -m toyslam_amd.build" % os.path.basename(path))
    return path


@pytest.fixture(scope="module")
def product_heads():
    return kh.heads(_built(build.HIP_SO), set(kh.HOT_KERNELS))


def test_every_hot_kernel_is_instantiated(product_heads):
    assert set(h.base for h in product_heads) == set(kh.HOT_KERNELS)
    assert len(kh.HOT_KERNELS) == 24


def test_hot_kernels_have_preloaded_arguments_and_wait_for_no_kernarg_load_before_their_first_vector_load(product_heads):
    bad = []
    for h in product_heads:
        if h.preload < 1:
            bad.append((h.symbol, "preload length", h.preload))
        exempt = h.base in EXEMPT and EXEMPT[h.base].search(h.symbol)
        if h.waited > (1 if exempt else 0):      # an exempt one waits for ONE load: the diagonal inverse's pointer
            bad.append((h.symbol, "kernarg loads waited for", h.waited))
    assert not bad, bad[:10]
    # an exemption that is no longer needed is taken off the list
    for base, rx in EXEMPT.items():
        assert any(h.waited for h in product_heads if h.base == base and rx.search(h.symbol)), base


def test_the_plain_library_preloads_nothing():
    hs = kh.heads(_built(build.HIP_PLAIN_SO))
    assert len(hs) > 500
    assert [h.symbol for h in hs if h.preload != 0] == []
    # ... and there the same kernels do wait for their arguments: the count is not zero by construction
    hot = [h for h in hs if h.base in kh.HOT_KERNELS]
    assert set(h.base for h in hot) == set(kh.HOT_KERNELS)
    assert [h.symbol for h in hot if h.waited == 0] == []
