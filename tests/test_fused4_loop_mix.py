"""k_fused4's row loops issue no more VALU slots per step than the stride-2 pair layout allows
(CPU check of the device assembly, tools/loop_mix.py; no GPU).

The kernel is bound by VALU issue, so what its loops carry besides the
arithmetic is its speed.  The layout's floor for a two-term loop is 198 issue slots per step
(132 pk_fma + 6 pk_mul + 18 horizontal blend + 12 straddling-pair assembly + 12 h2r + 12 bf16
unpack + 6 cvt_pk); the cap is 204, 6 for residue, s_nop included: a nop takes an issue slot
too.  The (even, odd) pair layout this replaced had 215.67-220.33 (profiles/r08/
fused4_loop_mix.txt), every loop of the new one is below its predecessor, and the three-term
loops (CD 0 / RC 0) stay at least 5 below theirs.

The assembly is built here with csrc/Makefile's flags for fused4.o; the test skips only where
hipcc is absent.  The same assembly goes through tools/dpp_hazard.py: no DPP operand is read
closer than 2 wait states to the VALU instruction that wrote it (the compiler's hazard
recognizer does not see the kernel's inline-asm packed ops as writers)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hybrid-grid-for-hexagonal-and-rectangular-image-processing_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
KERNELS = ("k_fused4ILi0", "k_fused4ILi1")
STEPS = 6                      # steps per loop trip (a 6-step block)
TWO_TERM_CAP = 204.0
# The parent's figures per loop in program order (profiles/r08/fused4_loop_mix.txt): loops 0-1
# the three-term ones, 2-9 the two-term ones.
PARENT = {
    "k_fused4ILi0": [238.00, 238.67, 220.33, 219.83, 219.00, 219.33, 216.83, 217.00, 215.67, 216.67],
    "k_fused4ILi1": [238.67, 240.17, 220.33, 219.83, 219.00, 219.50, 217.33, 217.00, 216.33, 218.00],
}

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc")


def _makefile_flags():
    """CXXFLAGS of csrc/Makefile plus what its fused4.o rule adds."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", mk, re.M).group(1).split()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)
    rule = re.search(r"^\$\(OBJDIR\)/fused4\.o: fused4\.hip.*\n(?:\t@.*\n)*\t\$\(HIPCC\)(.*)$", mk, re.M).group(1)
    extra = [t for t in rule.split() if t.startswith("-") and t not in ("-c", "-o")
             and not t.startswith("--offload-arch")]
    return [f"--offload-arch={arch}"] + flags + extra


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fused4") / "fused4.s")
    flags = _makefile_flags()
    assert "-fno-slp-vectorize" in flags and "-O3" in flags
    subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-S", "fused4.hip", "-o", out],
                   cwd=CSRC, check=True, stderr=subprocess.DEVNULL)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_row_loops_under_their_caps(asm, kernel):
    from loop_mix import row_loops
    loops = row_loops(asm, kernel, STEPS)
    figs = [round(f, 2) for _, _, _, f in loops]
    print(kernel, "figures per step:", figs, "parent:", PARENT[kernel])
    assert len(loops) == 10, "five (cd, rc) loops in each direction"
    pk = [c["pk"] for _, _, c, _ in loops]
    # the three-term loops come first and carry more packed blends than the two-term ones
    assert min(pk[:2]) > max(pk[2:]), pk
    for i, (fig, par) in enumerate(zip(figs, PARENT[kernel])):
        assert fig < par, (i, fig, par)
        if i < 2:
            assert fig <= par - 5, f"three-term loop {i}: {fig} > parent {par} - 5"
        else:
            assert fig <= TWO_TERM_CAP, f"two-term loop {i}: {fig} > {TWO_TERM_CAP}"


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_dpp_read_within_two_wait_states_of_its_writer(asm, kernel):
    from dpp_hazard import scan
    from loop_mix import kernel_lines
    _, body = kernel_lines(open(asm).read().splitlines(), kernel)
    bad, ndpp = scan(body, 2)
    assert ndpp > 500, "the kernel's DPP instructions were not found"
    assert not bad, bad[:5]


def test_resources_keep_three_waves_per_simd(asm):
    text = open(asm).read()
    vg = [int(v) for v in re.findall(r"\.vgpr_count:\s+(\d+)", text)]
    assert len(vg) == 2 and max(vg) <= 168, vg
    assert [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)] == [0, 0]
    assert [int(v) for v in re.findall(r"\.sgpr_spill_count:\s+(\d+)", text)] == [0, 0]
    assert [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)] == [0, 0]
