"""Host arithmetic of cs_attn's band walk (Options.csa_block_mb, csattn.hip csa_plan_bands): the band height and the workspace size as
the library's own exports name them -- no GPU.  Score storage per padded query row is Wp * Lld * 4 bytes of S plus, in the 16-bit
entries, Wp * Lld8 * 2 bytes of P16 (Lld / Lld8 = L rounded up to 4 / 8, L = (Hp / s)(Wp / s)); the four-block route keeps three halo
rows beside a band's own, and the smallest band is 8 logit rows (one item height of the box-sum scores; 4 in the 16-bit entries)."""
import ctypes as C

import pytest

from ciaosr_amd import _lib, hip_ops

MIB = 1 << 20
HALO, MIN_S_ROWS = 3, {0: 8, 1: 4, 2: 4}
F32, BF16, F16 = 0, 1, 2
# (H, W) -> bytes of S per padded query row, worked out by hand from csa_plan at scale 2
ROW_BYTES = {(64, 64): 256 * 1024, (67, 70): 70 * 1192 * 4, (192, 192): int(6.75 * MIB), (256, 256): 16 * MIB,
             (226, 340): 340 * 19212 * 4, (512, 512): 128 * MIB}


def _up(v, a):
    return (v + a - 1) // a * a


def _plan(H, W, scale=2):
    Hp, Wp = _up(H, scale), _up(W, scale)
    L = (Hp // scale) * (Wp // scale)
    return Hp, Wp, L, _up(L, 4), _up(L, 8)


def _rows(H, W, mb, precision=F32, C_=64, scale=2, **kw):
    opt = hip_ops.Options(csa_block_mb=mb, **kw)
    return _lib.load().ciaosr_cs_attn_block_rows(H, W, C_, scale, precision, opt.c_arg())


def _row_bytes(H, W, precision, scale=2):
    Hp, Wp, L, Lld, Lld8 = _plan(H, W, scale)
    return Wp * Lld * 4 + (Wp * Lld8 * 2 if precision != F32 else 0)


def _four_block(H, W, precision, C_=64, scale=2):
    """Where the four-block route is the preferred one: fp32, C = 64, scale 2, from 4096 padded pixels on, and its smallest band addressable."""
    Hp, Wp, L, Lld, _ = _plan(H, W, scale)
    return precision == F32 and C_ == 64 and scale == 2 and Hp * Wp >= 4096 and MIN_S_ROWS[F32] * Wp * Lld * 4 < 2 ** 31


@pytest.mark.parametrize('hw', sorted(ROW_BYTES))
def test_hand_worked_row_sizes(hw):
    assert _row_bytes(hw[0], hw[1], F32) == ROW_BYTES[hw]


def test_options_field_reaches_the_struct_and_negative_is_refused():
    opt = hip_ops.Options(csa_block_mb=256)
    assert opt.csa_block_mb == 256 and opt._c.csa_block_mb == 256 and 'csa_block_mb=256' in repr(opt)
    assert hip_ops.as_options(dict(csa_block_mb=3)).csa_block_mb == 3
    assert C.sizeof(_lib.OptionsT) == _lib.load().ciaosr_sizeof(b'ciaosr_options_t')
    assert _lib.OptionsT._fields_[-1][0] == 'csa_block_mb'
    lib = _lib.load()
    bad = hip_ops.Options(csa_block_mb=-1)
    assert lib.ciaosr_cs_attn_block_rows(64, 64, 64, 2, F32, bad.c_arg()) == 0
    assert lib.ciaosr_head_workspace_bytes_opt(8, 8, None, 4, bad.c_arg()) == 0
    # the entry point itself refuses it before it touches any pointer (options_ok): CIAOSR_ERR_BAD_ARG, no launch
    st = _lib.CsAttnWeightsT()
    st.channels, st.scale = 64, 2
    buf = C.create_string_buffer(64)
    rc = lib.ciaosr_cs_attn_f32(C.cast(buf, C.c_void_p), 64, 8, 8, C.byref(st), C.cast(buf, C.c_void_p), 64, bad.c_arg(),
                                C.cast(buf, C.c_void_p), 64, None)
    assert rc != 0 and b'argument' in lib.ciaosr_error_string(rc).lower()
    assert lib.ciaosr_version() >= 220


@pytest.mark.parametrize('precision', [F32, BF16, F16])
@pytest.mark.parametrize('hw', sorted(ROW_BYTES) + [(45, 51), (48, 48), (190, 187)])
def test_block_rows_is_hp_when_off_or_when_one_band_covers_the_map(hw, precision):
    H, W = hw
    Hp = _plan(H, W)[0]
    lib = _lib.load()
    assert lib.ciaosr_cs_attn_block_rows(H, W, 64, 2, precision, None) == Hp
    assert _rows(H, W, 0, precision) == Hp
    whole_mb = -(-_row_bytes(H, W, precision) * Hp // MIB)
    if whole_mb < 2 ** 31 // MIB * 1024:
        assert _rows(H, W, whole_mb, precision) == Hp
        assert _rows(H, W, whole_mb + 100, precision) == Hp


@pytest.mark.parametrize('precision', [F32, BF16, F16])
@pytest.mark.parametrize('kw', [{}, dict(csa_attn_v16=1), dict(csa_scores_gemm=1), dict(csa_composed_min=-1)], ids=str)
@pytest.mark.parametrize('hw', sorted(ROW_BYTES) + [(45, 51), (190, 187)])
def test_block_rows_grows_with_the_budget_and_stays_inside_it(hw, precision, kw):
    H, W = hw
    Hp, Wp, L, Lld, _ = _plan(H, W)
    row = _row_bytes(H, W, precision)
    four = _four_block(H, W, precision) and not kw.get('csa_attn_v16') and kw.get('csa_composed_min', 0) >= 0
    halo = HALO if four else 0
    budgets = sorted(set([1, 2, 3, 4, 7, 8, 16, 33, 64, 100, 128, 256, 500, 512, 1000, 1024, 1500, 2047, 2048, 3000, 4096, 6000, 8192, 16384]))
    last = 0
    for mb in budgets:
        rows = _rows(H, W, mb, precision, **kw)
        assert 1 <= rows <= Hp and rows >= last, (mb, rows, last)
        last = rows
        if rows == Hp:
            continue
        if mb * MIB >= MIN_S_ROWS[precision] * row:             # the budget admits the smallest band: a band with its halo stays inside it
            assert (rows + halo) * row <= mb * MIB, (mb, rows, halo, row)
        else:                                        # else that smallest band is what runs
            assert rows + halo == MIN_S_ROWS[precision], (mb, rows)
        s_band = (rows + halo) * Wp * Lld * 4
        assert s_band < (2 ** 31 if four else 0xFFFFFF00), (mb, rows, s_band)     # what the route's kernels address


def test_band_heights_of_the_documented_sizes():
    # 192 x 192, 6.75 MiB per row: 256 MiB hold 37 rows -> 32 (whole items of 8) -> 29 + 3 halo rows: 7 bands, the last one of 18 rows
    assert _rows(192, 192, 256) == 29 and _rows(192, 192, 100) == 14 - 3 and _rows(192, 192, 100, csa_attn_v16=1) == 14
    assert _rows(192, 192, 256, F16) == 24                         # 10.125 MiB per row with P16: 25 -> 24
    assert _rows(256, 256, 1024) == 64 - 3                         # 16 MiB per row
    assert _rows(226, 340, 512) == 16 - 3                          # 24.9 MiB per row: 20 -> 16
    assert _rows(512, 512, 1024) == 8 - 3 and _rows(512, 512, 2047) == 15 - 3       # 128 MiB per row; 2 GiB of S is 16 rows: one too many
    assert _rows(512, 512, 4096) == 15 - 3                         # the four-block route's 2 GiB, not the budget, bounds the band
    assert _rows(512, 512, 4096, csa_attn_v16=1) == 24             # the 16C route's 4 GiB: 31 rows -> 24
    assert _rows(512, 512, 512) == 8 - 3                           # below the smallest band: that band


@pytest.mark.parametrize('hw,mb', [((512, 512), 1024), ((226, 340), 512), ((256, 256), 1024), ((192, 192), 256), ((192, 192), 100)])
def test_workspace_bytes_opt_is_bounded_by_the_budget(hw, mb):
    H, W = hw
    lib = _lib.load()
    Hp, Wp, L, Lld, Lld8 = _plan(H, W)
    old = lib.ciaosr_cs_attn_workspace_bytes_scale(H, W, 64, 2)
    assert lib.ciaosr_cs_attn_workspace_bytes_opt(H, W, 64, 2, None) == old
    assert lib.ciaosr_cs_attn_workspace_bytes_opt(H, W, 64, 2, hip_ops.Options(csa_attn_v16=1).c_arg()) == old
    got = lib.ciaosr_cs_attn_workspace_bytes_opt(H, W, 64, 2, hip_ops.Options(csa_block_mb=mb).c_arg())
    bound = old - Hp * Wp * Lld * 4 - Hp * Wp * Lld8 * 2 + mb * MIB + (Hp + Wp) * Lld * 4 + 64 * 1024
    print(f'{H}x{W}, {mb} MiB: workspace {got / MIB:.0f} MiB (whole-map form {old / MIB:.0f} MiB, bound {bound / MIB:.0f} MiB)')
    assert 0 < got <= bound
    assert got >= (_rows(H, W, mb) + HALO) * Wp * Lld * 4           # and it does hold the fp32 band


def test_workspace_bytes_opt_equals_the_old_function_when_off():
    lib = _lib.load()
    for (H, W), sc in [((64, 64), 2), ((67, 70), 2), ((50, 47), 3), ((45, 54), 4), ((13, 9), 2)]:
        old = lib.ciaosr_cs_attn_workspace_bytes_scale(H, W, 64, sc)
        assert lib.ciaosr_cs_attn_workspace_bytes_opt(H, W, 64, sc, None) == old
        assert lib.ciaosr_cs_attn_workspace_bytes_opt(H, W, 64, sc, hip_ops.Options(csa_block_mb=0, csa_composed_min=1).c_arg()) == old
        assert lib.ciaosr_cs_attn_workspace_bytes_opt(H, W, 64, sc, hip_ops.Options(csa_block_mb=100000).c_arg()) == old


def test_restorer_test_cfg_reaches_the_option():
    from ciaosr_amd.restorer import CiaoSR
    opts = CiaoSR.options(type('R', (), dict(test_cfg=dict(scale=4, tile=192, hip_options=dict(csa_block_mb=1024))))())
    assert opts.csa_block_mb == 1024 and opts.precision == 'fp32'
