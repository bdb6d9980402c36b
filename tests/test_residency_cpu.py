"""CPU: the padding arithmetic of the residency table (csrc/residency.h) through the library's own entry point.

A cap is enforced by the launch alone: the launcher asks for so much dynamic LDS that exactly `cap` workgroups fit the 160 KiB of a CU
(requests are rounded up to 1280-byte granules by the hardware). For every covered kernel's footprint and every cap:
  * the padded workgroup admits exactly min(cap, what its own LDS admits) workgroups, never fewer than 1,
  * the padding is the smallest such (one granule less would admit cap + 1), so the rest of the CU stays free for the partner kernel,
  * cap 0 asks for nothing extra, and neither does a cap the kernel's own LDS already enforces.
"""
import pytest

LDS_PER_CU = 160 * 1024
GRANULE = 1280
MAX_CAP = 8

# (kernel, static LDS, dynamic LDS) of every covered launch configuration, from the launchers:
FOOTPRINTS = [
    ("conv1x1_frag", 0, 2 * 8 * 64 * 16),                                  # two A buffers of 8 quarters x 64 pixels x 16 bytes
    ("conv1x1_pair res2", 0, (8 * (64 // 32) + 32) * 65 * 16),             # x tile + 128-channel chunk, pitch 65
    ("conv1x1_pair res3", 0, (8 * (128 // 32) + 32) * 65 * 16),
    ("conv1x1_pair32 8 waves", 0, (8 * (256 // 32) + 64) * 33 * 16),       # pitch 33
    ("conv1x1_pair32 4 waves", 0, (8 * (256 // 32) + 32) * 33 * 16),
    ("conv1x1_ksw 16x64", 4 * 16 * 1 * (64 + 4) * 4, 0),                   # `red`: 4 waves x 16 PRB rows x (16 CB + 4) floats
    ("conv1x1_ksw 32x32", 4 * 16 * 2 * (32 + 4) * 4, 0),
    ("conv1x1_ksw 32x64", 4 * 16 * 2 * (64 + 4) * 4, 0),
    ("conv1x1_ksw 64x64", 4 * 16 * 2 * (64 + 4) * 4, 0),
    ("conv_wino16<32,64>", 0, 2 * 16 * 4 * 32 * 16),
    ("conv_wino16<32,32>", 0, 2 * 16 * 4 * 32 * 16),
    ("dcn_fused 3x3", 0, 2 * 8 * 65 * 16 + 9 * 64 * 36),                   # two A buffers, pitch 65, + 36 bytes per tap and pixel
    ("dcn_fused 1x1", 0, 2 * 8 * 65 * 16 + 1 * 64 * 36),
]


def admitted(total):
    """Workgroups of `total` bytes of LDS the hardware places on one CU."""
    return LDS_PER_CU // (-(-total // GRANULE) * GRANULE)


@pytest.fixture(scope="module")
def pad():
    from upsnet_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib().upsnet_residency_pad_bytes


@pytest.mark.parametrize("name,static,dynamic", FOOTPRINTS, ids=[f[0] for f in FOOTPRINTS])
def test_padding_admits_exactly_the_cap(pad, name, static, dynamic):
    own = admitted(static + dynamic)
    assert own >= 1
    assert pad(0, static, dynamic) == 0
    for cap in range(1, MAX_CAP + 1):
        extra = pad(cap, static, dynamic)
        total = static + dynamic + extra
        assert total <= LDS_PER_CU, (name, cap, total)
        assert admitted(total) == min(cap, own) >= 1, (name, cap, extra, admitted(total))
        if cap >= own:
            assert extra == 0, (name, cap, extra)                          # the kernel's own LDS already holds it there
        else:
            assert extra > 0 and total % GRANULE == 0
            assert admitted(total - GRANULE) == cap + 1, (name, cap, extra)   # the smallest request that does it


def test_tuning_call_validates_and_resets():
    from upsnet_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.lib()
    try:
        assert lib.upsnet_residency_tuning(7, 1) != 0 and b"kernel" in lib.upsnet_last_error()
        assert lib.upsnet_residency_tuning(0, MAX_CAP + 1) != 0 and b"cap" in lib.upsnet_last_error()
        assert lib.upsnet_residency_tuning(0, -2) != 0
        for k in range(-1, 7):
            for cap in (-1, 0, 1, MAX_CAP):
                assert lib.upsnet_residency_tuning(k, cap) == 0
    finally:
        assert lib.upsnet_residency_tuning(-1, 0) == 0
