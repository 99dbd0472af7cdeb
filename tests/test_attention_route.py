"""Which attention kernels a map takes (ops.attention_route), and the UNet's input-size check above 4096 attention
pixels: CPU only."""
import pytest

from view_fusion_amd import UNet
from view_fusion_amd.ops import attention_route

TINY3 = dict(in_channel=6, out_channel=6, inner_channel=32, norm_groups=32, channel_mults=(1, 2, 2), attn_res=(4,),
             res_blocks=1, image_size=16)
# attention on level 0 (attn_res = image_size); the mid block adds attention on level 1
ATTN0 = dict(in_channel=6, out_channel=6, inner_channel=32, norm_groups=32, channel_mults=(1, 2), attn_res=(16,),
             res_blocks=1, image_size=16)


def _route_before(C, L):
    # the choice ops.attention made before the streaming kernels existed, for every L it accepted
    return "fused" if L in (64, 256) and C % 32 == 0 else "generic"


@pytest.mark.parametrize("C", [8, 32, 48, 64, 96, 128, 320, 512])
def test_route_unchanged_up_to_4096(C):
    for L in list(range(1, 300)) + [576, 1024, 1296, 2304, 3600, 4032, 4095, 4096]:
        assert attention_route(C, L) == _route_before(C, L), (C, L)


@pytest.mark.parametrize("C", [8, 48, 64, 320, 512])
def test_route_streams_above_4096(C):
    for L in (4097, 4356, 5120, 5184, 9216, 16384, 65536):
        assert attention_route(C, L) == "stream", (C, L)


def test_check_input_size_accepts_large_attention_maps():
    net = UNet(**ATTN0)
    assert net._vf_attn_levels == (0, 1)
    for H, W in ((72, 72), (128, 128), (64, 80), (96, 96)):
        net.check_input_size(H, W)


def test_check_input_size_still_rejects_outside_the_reference_envelope():
    with pytest.raises(ValueError, match="18x18"):
        UNet(**TINY3).check_input_size(18, 18)
    with pytest.raises(ValueError, match="72x74"):
        UNet(**TINY3).check_input_size(72, 74)
