"""The per-image trunk drivers (ciaosr_swinir_forward_f32, csrc/swinir.hip; ciaosr_edsr_forward_f32, csrc/encoder.hip), everything that
needs no GPU: the byte counts of their carve lists against the closed forms the entries were first written with, and their refusals --
every one of them before the first memset or launch.  The structs hold fake device pointers that are never dereferenced; without a GPU
anything that reached a memset or a launch would come back as CIAOSR_ERR_LAUNCH, so a CIAOSR_ERR_BAD_ARG here IS "refused first"."""
import ctypes as C

import pytest

from ciaosr_amd import _lib
from tests.test_swinir_h16_host import _Fake as _FakeSwin

ERR_BAD_ARG, ERR_WORKSPACE = -1, -4
P = 0x10000                                                # 16-byte aligned, never read
SIZES = ((48, 48), (45, 51), (8, 64), (192, 192))


def _up(v, a):
    return (v + a - 1) // a * a


# ---- SwinIR fp32 -------------------------------------------------------------------------------------------------------------------
def _swin(C_=180, heads=6, hidden=360, groups=2, depth=2):
    return _FakeSwin(C_=C_, heads=heads, hidden=hidden, groups=groups, depth=depth, w16=False)


def _swin_bytes(f, H, W):
    return _lib.load().ciaosr_swinir_workspace_bytes(H, W, C.byref(f.st))


def _swin_forward(f, H, W, ws_bytes=None):
    n = _swin_bytes(f, H, W) if ws_bytes is None else ws_bytes
    return _lib.load().ciaosr_swinir_forward_f32(P, H, W, C.byref(f.st), P, P, n, None)


@pytest.mark.parametrize('C_,hidden', [(180, 360), (60, 120)])
def test_swinir_workspace_bytes_is_the_closed_form(C_, hidden):
    f = _swin(C_=C_, hidden=hidden)
    ld, ldh, ldq = _up(C_, 64), _up(hidden, 64), _up(3 * C_, 32)
    for H, W in SIZES:
        HW = _up(H, 8) * _up(W, 8)
        # image, patch rows, x0 + two token maps + normed + attention, QKV, hidden, split-K slabs
        floats = HW * 4 + HW * 36 + 5 * HW * ld + HW * ldq + HW * ldh + 16 * HW * ld
        assert _swin_bytes(f, H, W) == floats * 4 + 16 * 256, (C_, H, W)


def test_swinir_workspace_bytes_zero_for_bad_arguments():
    lib, f = _lib.load(), _swin()
    assert lib.ciaosr_swinir_workspace_bytes(48, 48, None) == 0
    assert _swin_bytes(f, 0, 48) == 0 and _swin_bytes(f, 48, 0) == 0 and _swin_bytes(f, -8, 48) == 0 and _swin_bytes(f, 48, -3) == 0
    f.st.window_size = 0
    assert _swin_bytes(f, 48, 48) == 0


def test_swinir_forward_refuses_before_any_launch():
    assert _swin_forward(_swin(C_=90, heads=3, hidden=180), 48, 48) == ERR_BAD_ARG     # C not a multiple of 4
    assert _swin_forward(_swin(heads=12), 48, 48) == ERR_BAD_ARG                       # head dimension 15: odd
    assert _swin_forward(_swin(heads=5), 48, 48) == ERR_BAD_ARG                        # head dimension 36 > 32
    assert _swin_forward(_swin(), 4, 48) == ERR_BAD_ARG                                # reflect padding needs pad < size
    assert _swin_forward(_swin(), 48, 4) == ERR_BAD_ARG
    f = _swin()
    f.st.norm_w = None
    assert _swin_forward(f, 48, 48) == ERR_BAD_ARG
    # the defects the entry used to find only after the earlier blocks and groups were on the stream
    for name in ('ln1_w', 'qkv_w', 'qkv_b', 'bias', 'proj_w', 'ln2_b', 'fc1_w', 'fc2_w', 'fc2_b'):
        f = _swin()
        setattr(f.blocks[-1], name, None)                                              # a missing pointer in the LAST block
        assert _swin_forward(f, 48, 48) == ERR_BAD_ARG, name
    f = _swin()
    f.blocks[-1].shift = 4                                                             # a shifted LAST block without its mask
    assert _swin_forward(f, 48, 48) == ERR_BAD_ARG
    f = _swin()
    f.gconv[-1].cin = 180                                                              # the LAST group_conv: cin is not ld
    assert _swin_forward(f, 48, 48) == ERR_BAD_ARG
    f = _swin()
    f.gconv[-1].bias = None
    assert _swin_forward(f, 48, 48) == ERR_BAD_ARG


def test_swinir_forward_short_workspace():
    f = _swin()
    for H, W in ((48, 48), (45, 51)):
        assert _swin_forward(f, H, W, ws_bytes=_swin_bytes(f, H, W) - 1) == ERR_WORKSPACE
    assert _swin_forward(f, 48, 48, ws_bytes=0) == ERR_WORKSPACE


# ---- EDSR per image ------------------------------------------------------------------------------------------------------------------
class _FakeEdsr:
    def __init__(self, C_=64, blocks=2):
        st = _lib.EdsrWeightsT()
        st.mid_channels, st.num_blocks, st.res_scale = C_, blocks, 1.0
        convs = [st.conv_first, st.conv_after_body]
        if blocks:
            self.c1, self.c2 = (_lib.ConvT * blocks)(), (_lib.ConvT * blocks)()
            st.conv1, st.conv2 = self.c1, self.c2
            convs += list(self.c1) + list(self.c2)
        for cv in convs:
            cv.weight, cv.bias, cv.cin, cv.cout, cv.ksize = P, P, C_, C_, 3
        st.conv_first.cin = 3
        self.st = st

    def bytes(self, H, W):
        return _lib.load().ciaosr_edsr_workspace_bytes(H, W, C.byref(self.st))

    def forward(self, H, W, ws_bytes=None):
        n = self.bytes(H, W) if ws_bytes is None else ws_bytes
        return _lib.load().ciaosr_edsr_forward_f32(P, H, W, C.byref(self.st), P, P, n, None)


@pytest.mark.parametrize('C_', [64, 32])
def test_edsr_workspace_bytes_is_the_closed_form(C_):
    f = _FakeEdsr(C_=C_)
    for H, W in SIZES:
        HW = H * W
        # image, patch rows, first + two block outputs + conv1's output, split-K slabs
        assert f.bytes(H, W) == (HW * 4 + HW * 36 + 4 * HW * C_ + 16 * HW * C_) * 4 + 16 * 256, (C_, H, W)


def test_edsr_workspace_bytes_zero_for_bad_arguments():
    f = _FakeEdsr()
    assert _lib.load().ciaosr_edsr_workspace_bytes(48, 48, None) == 0
    assert f.bytes(0, 48) == 0 and f.bytes(48, 0) == 0 and f.bytes(-1, 48) == 0 and f.bytes(48, -1) == 0


def test_edsr_forward_refuses_before_any_launch():
    for which, field, value in (('c1', 'cin', 32), ('c2', 'cout', 32), ('c1', 'weight', None), ('c2', 'bias', None), ('c2', 'ksize', 1)):
        f = _FakeEdsr(blocks=3)
        setattr(getattr(f, which)[-1], field, value)                                   # the LAST block's conv1 / conv2
        assert f.forward(19, 24) == ERR_BAD_ARG, (which, field)
    f = _FakeEdsr()
    f.st.conv_after_body.cin = 32
    assert f.forward(19, 24) == ERR_BAD_ARG
    f = _FakeEdsr(C_=48)                                                               # not a multiple of 32
    assert f.forward(19, 24) == ERR_BAD_ARG
    f = _FakeEdsr()
    f.st.conv1 = None                                                                  # blocks without their convolutions
    assert f.forward(19, 24) == ERR_BAD_ARG


def test_edsr_forward_short_workspace_and_no_blocks():
    f = _FakeEdsr()
    for H, W in ((19, 24), (48, 48)):
        assert f.forward(H, W, ws_bytes=f.bytes(H, W) - 1) == ERR_WORKSPACE
    # NB = 0 with null conv1 / conv2 passes the argument checks: the workspace check, which comes after them, is what answers (and the
    # route export, which runs the same checks, reports route 0)
    g = _FakeEdsr(blocks=0)
    assert not g.st.conv1 and not g.st.conv2
    assert g.forward(19, 24, ws_bytes=g.bytes(19, 24) - 1) == ERR_WORKSPACE
    assert _lib.load().ciaosr_edsr_route_code(1, 19, 24, C.byref(g.st), None) == 0
