"""What the compiler made of the halo-DMA instantiations of vpt_conv3x3_kernel (no GPU needed; tests/test_kernel_resources_cpu.py matches the
16-row kernels by the END of their mangled name, which the fourth template parameter moves): modes 0, 1, 4 and 5 exist in both operand formats,
stay within 256 VGPRs with no spill and no scratch, and their 79 424 bytes of LDS leave room for two workgroups per CU."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc (the build container); the GPU box runs the prebuilt libraries")


@pytest.mark.parametrize("tag", ["bf16", "f16"])
def test_halo_dma_kernels_fit_two_workgroups_per_cu(tag):
    spec = importlib.util.spec_from_file_location("_vpt_build_hdma", os.path.join(ROOT, "video-pre-training_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    res = {k: v for k, v in mod.kernel_resources(tag).items() if "vpt_conv3x3_kernel" in k and "ELi16ELb1EE" in k}
    assert sorted(k.split("ILb0ELi")[1][0] for k in res) == ["0", "1", "4", "5"], sorted(res)
    for k, v in res.items():
        assert v["vgprs"] <= 256 and v["agprs"] == 0 and not v["vgpr_spill"] and not v["sgpr_spill"] and not v["scratch"], (k, v)
        assert v["occupancy"] >= 2 and v["lds"] == 79424 and 2 * v["lds"] <= 160 * 1024, (k, v)
