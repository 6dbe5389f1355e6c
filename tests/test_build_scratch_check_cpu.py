"""rscotr_amd.build.scratch_report: the build reads hipcc's kernel-resource-usage remarks of the kernels that must not spill."""
from rscotr_amd.build import NO_SCRATCH, scratch_report

REMARKS = """\
a.hip:16:1: remark: Function Name: _ZN6rscotr18gemm_h3_128_kernelILb1ELb1ELb0ELb0EEEvNS_10GemmParamsE [-Rpass-analysis=kernel-resource-usage]
a.hip:16:1: remark:     VGPRs: 249 [-Rpass-analysis=kernel-resource-usage]
a.hip:16:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]
a.hip:9:1: remark: Function Name: _ZN6rscotr14gemm_h3_kernelILi64ELi64ELb0ELb0ELi2ELb0ELi4ELb1EEEvNS_10GemmParamsE [-Rpass-analysis=kernel-resource-usage]
a.hip:9:1: remark:     ScratchSize [bytes/lane]: 24 [-Rpass-analysis=kernel-resource-usage]
a.hip:16:1: remark: Function Name: _ZN6rscotr18gemm_h3_128_kernelILb1ELb1ELb1ELb0EEEvNS_10GemmParamsE [-Rpass-analysis=kernel-resource-usage]
a.hip:16:1: remark:     ScratchSize [bytes/lane]: 12 [-Rpass-analysis=kernel-resource-usage]
"""


def test_scratch_report_names_the_kernels_that_spill():
    rep = scratch_report(REMARKS, NO_SCRATCH['gemm_h3.hip'])
    assert rep == {'_ZN6rscotr18gemm_h3_128_kernelILb1ELb1ELb0ELb0EEEvNS_10GemmParamsE': 0,
                   '_ZN6rscotr18gemm_h3_128_kernelILb1ELb1ELb1ELb0EEEvNS_10GemmParamsE': 12}
    assert scratch_report('', NO_SCRATCH['gemm_group.hip']) == {}
