"""The opt-in EDSR trunk over tile batches (Options.edsr_resident -> ciaosr_edsr_forward_batch_f32, csrc/encoder.hip on the halo-resident
kernel of csrc/dense_f32.hip), everything that needs no GPU: the option and the three exports, the route rule of ciaosr_edsr_route_code on
weight structs whose device pointers are never dereferenced (the function launches nothing), the workspace sizes, and the restorer's
default tile_batch."""
import ctypes as C

from ciaosr_amd import _lib, hip_ops

P = 0x10000                  # 16-byte aligned, never read
HW_BIG = (192, 192)          # 256 tiles of 12 x 12 pixels
HW_SMALL = (48, 48)          # 16 tiles: under the default dense_min_tiles = 128
ON = dict(edsr_resident=1)


class _Fake:
    """An EDSR weight struct of host fields and fake device pointers."""

    def __init__(self, C_=64, blocks=16, frag=True):
        st = _lib.EdsrWeightsT()
        st.mid_channels, st.num_blocks, st.res_scale = C_, blocks, 1.0

        def fill(cv, cin):
            cv.weight, cv.bias, cv.cin, cv.cout, cv.ksize = P, P, cin, C_, 3
            cv.frag = P if frag and cin == C_ else None

        fill(st.conv_first, 3)
        fill(st.conv_after_body, C_)
        self.c1 = (_lib.ConvT * max(blocks, 1))()
        self.c2 = (_lib.ConvT * max(blocks, 1))()
        for i in range(blocks):
            fill(self.c1[i], C_)
            fill(self.c2[i], C_)
        st.conv1, st.conv2 = self.c1, self.c2
        self.st = st

    def route(self, B, hw, opt=None):
        return _lib.load().ciaosr_edsr_route_code(B, hw[0], hw[1], C.byref(self.st), hip_ops.as_options(opt).c_arg())

    def bytes(self, B, hw, opt=None):
        return _lib.load().ciaosr_edsr_workspace_bytes_batch(B, hw[0], hw[1], C.byref(self.st), hip_ops.as_options(opt).c_arg())


def test_option_and_abi_surface():
    lib = _lib.load()
    o = hip_ops.Options(edsr_resident=1)
    assert o.edsr_resident == 1 and o._c.edsr_resident == 1 and 'edsr_resident=1' in repr(o)
    assert hip_ops.Options().edsr_resident == 0 and 'edsr_resident' not in repr(hip_ops.Options('f16'))
    assert hip_ops.Options('f16', edsr_resident=1).replace(query_grid_w=3).edsr_resident == 1
    assert [f[0] for f in _lib.OptionsT._fields_[-3:]] == ['edsr_resident', 'swin_h16', 'csa_block_mb']
    assert hip_ops.Options._C_FIELDS[-3:] == ('edsr_resident', 'swin_h16', 'csa_block_mb')
    assert C.sizeof(_lib.OptionsT) == lib.ciaosr_sizeof(b'ciaosr_options_t') > 0
    assert lib.ciaosr_version() >= 260
    for name in ('ciaosr_edsr_workspace_bytes_batch', 'ciaosr_edsr_route_code', 'ciaosr_edsr_forward_batch_f32'):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    # out of range: an entry that reads the option refuses it
    f = _Fake()
    assert f.bytes(1, HW_BIG, dict(edsr_resident=2)) == 0
    assert f.route(1, HW_BIG, dict(edsr_resident=2)) < 0
    # the old entries are where they were
    assert lib.ciaosr_edsr_workspace_bytes(48, 48, C.byref(f.st)) > 0 and hasattr(lib, 'ciaosr_edsr_forward_f32')


def test_route_code_follows_the_rule():
    f = _Fake()
    assert f.route(1, HW_BIG) == 0 and f.route(4, HW_BIG) == 0                    # opt == NULL
    assert hip_ops.Options().c_arg() is None
    assert f.route(4, HW_BIG, dict(dense_min_tiles=1)) == 0                       # options without the field
    assert f.route(1, HW_BIG, ON) == 1 and f.route(8, HW_BIG, ON) == 1
    assert f.route(1, HW_SMALL, ON) == 0                                          # 16 tiles < 128
    assert f.route(3, HW_SMALL, dict(edsr_resident=1, dense_min_tiles=1)) == 1
    assert f.route(3, HW_SMALL, dict(edsr_resident=1, dense_min_tiles=16)) == 1 and f.route(3, HW_SMALL, dict(edsr_resident=1, dense_min_tiles=17)) == 0
    assert f.route(3, HW_BIG, dict(edsr_resident=1, dense_min_tiles=-1)) == 0     # never
    assert _Fake(C_=32).route(2, HW_BIG, ON) == 0
    assert _Fake(C_=128).route(2, HW_BIG, ON) == 0
    assert _Fake(blocks=0).route(2, HW_BIG, ON) == 0
    assert _Fake(frag=False).route(2, HW_BIG, ON) == 0
    for which in ('c1', 'c2'):
        one = _Fake()
        getattr(one, which)[7].frag = None
        assert one.route(2, HW_BIG, ON) == 0, which
    one = _Fake()
    one.st.conv_after_body.frag = None
    assert one.route(2, HW_BIG, ON) == 0
    # bad arguments: the error the call would return
    assert f.route(0, HW_BIG, ON) == -1 and f.route(1, (0, 5), ON) == -1
    bad = _Fake()
    bad.c2[3].cin = 32
    assert bad.route(1, HW_BIG, ON) == -1
    assert _lib.load().ciaosr_edsr_route_code(1, 8, 8, None, None) == -1


def test_a_batch_past_32_bit_offsets_runs_in_sub_batches():
    """[B HW][128] fp32 past 4 GiB - 256 B with B > 1: still resident, bits 8.. of the code = the images per pass; a single image past
    it goes per image."""
    f = _Fake()
    img = HW_BIG[0] * HW_BIG[1] * 128 * 4
    fit = (0xFFFFFF00 - 1) // img
    assert fit == 227
    assert f.route(fit, HW_BIG, ON) == 1
    code = f.route(fit + 1, HW_BIG, ON)
    assert code & 0xFF == 1 and code >> 8 == fit
    assert f.route(300, HW_BIG, ON) == 1 | fit << 8
    assert f.bytes(300, HW_BIG, ON) == f.bytes(fit, HW_BIG, ON) > fit * img                  # a pass at a time
    assert 2896 * 2896 * 512 < 0xFFFFFF00 <= 2897 * 2897 * 512
    assert f.route(1, (2896, 2896), ON) == 1 and f.route(2, (2896, 2896), ON) == 1 | 1 << 8  # one image per pass
    assert f.route(1, (2897, 2897), ON) == 0 and f.route(2, (2897, 2897), ON) == 0           # one image does not fit: per image


def test_workspace_bytes():
    lib = _lib.load()
    f = _Fake()
    for hw in (HW_BIG, HW_SMALL, (19, 70)):
        old = lib.ciaosr_edsr_workspace_bytes(hw[0], hw[1], C.byref(f.st))
        assert f.bytes(1, hw) == old > 0                                          # opt == NULL, B = 1
        assert f.bytes(5, hw) == old                                              # route 0: one image after the other
    assert f.bytes(5, HW_SMALL, ON) == lib.ciaosr_edsr_workspace_bytes(48, 48, C.byref(f.st))
    for hw, opt in ((HW_BIG, ON), (HW_SMALL, dict(edsr_resident=1, dense_min_tiles=1)), ((19, 70), dict(edsr_resident=1, dense_min_tiles=1))):
        sizes = [f.bytes(B, hw, opt) for B in range(1, 10)]
        assert all(b > a for a, b in zip(sizes, sizes[1:])), sizes
        px = hw[0] * hw[1]
        assert sizes[0] >= px * (4 + 36 + 64 + 128) * 4 and sizes[1] - sizes[0] == px * (64 + 128) * 4
    assert f.bytes(0, HW_BIG, ON) == 0 and f.bytes(1, (0, 4), ON) == 0
    assert lib.ciaosr_edsr_workspace_bytes_batch(1, 8, 8, None, None) == 0


def test_forward_refuses_before_any_launch():
    lib = _lib.load()
    f = _Fake()
    on = hip_ops.Options(edsr_resident=1)
    call = lambda B, hw, n, opt: lib.ciaosr_edsr_forward_batch_f32(P, B, hw[0], hw[1], C.byref(f.st), P, opt, P, n, None)
    assert call(0, HW_BIG, 1 << 40, on.c_arg()) == -1
    assert call(2, HW_BIG, f.bytes(2, HW_BIG, ON) - 1, on.c_arg()) == -4
    assert call(2, HW_BIG, f.bytes(1, HW_BIG, ON), on.c_arg()) == -4
    assert call(2, HW_BIG, 1 << 40, hip_ops.Options(edsr_resident=2).c_arg()) == -1
    assert call(2, HW_SMALL, 0, None) == -4


def _edsr_restorer(test_cfg):
    from ciaosr_amd import CiaoSR, LocalImplicitSREDSR
    mk = lambda i, o: dict(type='MLPRefiner', in_dim=i, out_dim=o, hidden_list=[32, 32])
    gen = dict(type=LocalImplicitSREDSR, encoder=dict(type='EDSR', in_channels=3, out_channels=3, mid_channels=64, num_blocks=2),
               imnet_q=mk(4, 3), imnet_k=mk(64, 64), imnet_v=mk(64, 64), feat_unfold=True, eval_bsize=30000)
    return CiaoSR(generator=gen, pixel_loss=dict(type='L1Loss'), test_cfg=test_cfg).eval()


def test_tile_batch_default_under_the_option():
    from ciaosr_amd.restorer import EDSR_TILE_BATCH, trunk_batches
    assert EDSR_TILE_BATCH == 8
    m = _edsr_restorer(dict(scale=4, tile=192, tile_overlap=32, hip_options=dict(edsr_resident=1)))
    assert m.options().edsr_resident == 1 and trunk_batches(m.generator, m.options())
    assert m.tile_batch() == 8
    for prec in ('f16', 'bf16', 'f16x3', 'bf16-single'):
        m.test_cfg['precision'] = prec
        assert m.options().edsr_resident == 1 and m.tile_batch() == 8, prec
    m.test_cfg['tile_batch'] = 3
    assert m.tile_batch() == 3
    m.test_cfg.pop('tile_batch')
    # option off: what it was (7 where the RDN rule says 7: fp32 with dense_direct = 0, a 16-bit trunk with dense_direct != 1)
    m.test_cfg.pop('hip_options')
    m.test_cfg.pop('precision')
    assert m.tile_batch() == 7
    m.test_cfg['precision'] = 'f16'
    assert m.tile_batch() == 7
    m.test_cfg['hip_options'] = dict(dense_direct=1)
    assert m.tile_batch() == 8
    m.test_cfg['precision'] = 'fp32'
    assert m.tile_batch() == 8
    m.test_cfg['hip_options'] = dict(edsr_resident=0)
    assert m.tile_batch() == 7
    # the option names the EDSR trunk alone: an RDN restorer keeps its rule
    from ciaosr_amd import CiaoSR, LocalImplicitSRRDN
    mk = lambda i, o: dict(type='MLPRefiner', in_dim=i, out_dim=o, hidden_list=[32, 32])
    gen = dict(type=LocalImplicitSRRDN, encoder=dict(type='RDN', in_channels=3, out_channels=3, mid_channels=64, num_blocks=1, upscale_factor=4,
                                                      num_layers=2, channel_growth=64),
               imnet_q=mk(4, 3), imnet_k=mk(64, 64), imnet_v=mk(64, 64), feat_unfold=True, eval_bsize=30000)
    r = CiaoSR(generator=gen, pixel_loss=dict(type='L1Loss'), test_cfg=dict(scale=4, tile=192, tile_overlap=32, hip_options=dict(edsr_resident=1))).eval()
    assert r.tile_batch() == 7
