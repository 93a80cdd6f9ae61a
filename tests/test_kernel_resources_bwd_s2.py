"""k_hexconv_bwd_weight_mfma_s2 (csrc/conv_mfma_bwd.hip) uses no scratch and spills no VGPRs:
tests/test_kernel_resources.py's code-object reader applied to the stride-2 d kernel GEMM, every
instantiation (three input dtypes x 2 and 4 output-channel tiles).  SGPR spills are printed."""
import os
import shutil
import sys

import pytest

import test_kernel_resources as KR


@pytest.mark.skipif(not os.path.exists(KR.LIB) or shutil.which("objcopy") is None
                    or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readobj"),
                    reason="needs the built library and the ROCm LLVM tools")
def test_stride2_weight_gradient_kernel_resources():
    sys.path.insert(0, os.path.join(KR.ROOT, "tools"))
    from kernel_resources import resources
    res = {k: v for k, v in resources(KR.LIB).items() if "k_hexconv_bwd_weight_mfma_s2" in k}
    assert len(res) == 6, sorted(res)
    assert {KR._family(k) for k in res} == {"k_hexconv_bwd_weight_mfma_s2"}
    for k, (scratch, sgpr_spills, vgpr_spills) in sorted(res.items()):
        print(f"{scratch} B scratch, {sgpr_spills} sgpr spills, {vgpr_spills} vgpr spills  {k}")
        assert scratch == 0 and vgpr_spills == 0, k
    # the stride-1 sibling kept its instantiations
    assert len([k for k in resources(KR.LIB) if "k_hexconv_bwd_weight_mfmaI" in k]) == 6
