"""Host tests of the Deep Zoom pyramid (ciaosr_amd/pyramid.py, CiaoSR.render_pyramid's argument checks, tools/render.py --dzi) and of the
ABI surface of the tile-batched PNG encoder.  No device work."""
import ctypes as C
import os
import re

import pytest
import torch

from ciaosr_amd import pyramid

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(REPO, 'configs', '001_localimplicitsr_edsr_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py')


def _cols(level):
    return sorted({(t[3], t[5]) for t in level['tiles']})


def _rows(level):
    return sorted({(t[2], t[4]) for t in level['tiles']})


def test_plan_against_hand_computed_values():
    plan = pyramid.dzi_plan(300, 600, 254, 1)                   # 600 wide, 300 high
    assert len(plan) == 11 and [lv['level'] for lv in plan] == list(range(11))
    top = plan[10]
    assert (top['height'], top['width']) == (300, 600) and len(top['tiles']) == 6
    assert _cols(top) == [(0, 255), (253, 256), (507, 93)]
    assert _rows(top) == [(0, 255), (253, 47)]
    assert [(t[0], t[1]) for t in top['tiles']] == [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1)]          # (col, row), row-major
    assert top['tiles'][4] == (1, 1, 253, 253, 47, 256)
    nine = plan[9]
    assert (nine['height'], nine['width']) == (150, 300)
    assert _cols(nine) == [(0, 255), (253, 47)] and _rows(nine) == [(0, 150)]
    assert (plan[0]['height'], plan[0]['width']) == (1, 1) and plan[0]['tiles'] == [(0, 0, 0, 0, 1, 1)]
    one = pyramid.dzi_plan(1, 1)
    assert len(one) == 1 and one[0] == dict(level=0, height=1, width=1, tiles=[(0, 0, 0, 0, 1, 1)])
    assert [(lv['width'], lv['height']) for lv in pyramid.dzi_plan(3, 5)] == [(1, 1), (2, 1), (3, 2), (5, 3)]
    assert pyramid.level_sizes(5424, 8160)[-1] == (5424, 8160) and len(pyramid.level_sizes(5424, 8160)) == 14


def _brute_levels(h, w):
    """Deep Zoom's rule restated: halve (rounding up) from the top until both sides are 1; exactly ceil(log2(max)) halvings."""
    sizes = [(h, w)]
    while max(sizes[0]) > 1:
        sizes.insert(0, ((sizes[0][0] + 1) // 2, (sizes[0][1] + 1) // 2))
    return sizes


def _brute_spans(n, t, o):
    out = []
    c = 0
    while c * t < n:
        lo = max(0, c * t - o)
        hi = min(n, c * t + t + o)
        out.append((lo, hi - lo))
        c += 1
    return out


@pytest.mark.parametrize('t,o', [(1, 0), (2, 0), (3, 1), (4, 3), (7, 2), (16, 1), (254, 1), (40, 0), (41, 5)])
def test_plan_against_a_brute_force_restatement(t, o):
    for h, w in [(1, 1), (1, 40), (40, 1), (2, 3), (7, 5), (16, 16), (17, 33), (31, 32), (33, 32), (40, 40), (39, 23)]:
        plan = pyramid.dzi_plan(h, w, t, o)
        sizes = _brute_levels(h, w)
        assert [(lv['height'], lv['width']) for lv in plan] == sizes, (h, w)
        for lv in plan:
            hl, wl = lv['height'], lv['width']
            cols, rows = _brute_spans(wl, t, o), _brute_spans(hl, t, o)
            assert lv['tiles'] == [(c, r, y0, x0, hh, ww) for r, (y0, hh) in enumerate(rows) for c, (x0, ww) in enumerate(cols)]
            cover = [[0] * wl for _ in range(hl)]                       # the tiles minus their overlaps partition the level
            for c, r, y0, x0, hh, ww in lv['tiles']:
                assert hh >= 1 and ww >= 1 and y0 >= 0 and x0 >= 0 and y0 + hh <= hl and x0 + ww <= wl
                ya, xa = (y0 + o if r > 0 else y0), (x0 + o if c > 0 else x0)
                yb, xb = min(hl, (r + 1) * t), min(wl, (c + 1) * t)
                assert (ya, xa) == (r * t, c * t) and yb <= y0 + hh and xb <= x0 + ww
                for y in range(ya, yb):
                    for x in range(xa, xb):
                        cover[y][x] += 1
            assert all(v == 1 for row in cover for v in row), (h, w, lv['level'])


def test_manifest_and_value_errors():
    assert pyramid.dzi_manifest(300, 600, 254, 1) == (
        '<?xml version="1.0" encoding="UTF-8"?><Image xmlns="http://schemas.microsoft.com/deepzoom/2008" Format="png" Overlap="1" '
        'TileSize="254"><Size Width="600" Height="300"/></Image>')
    assert 'Overlap="0" TileSize="16"><Size Width="5" Height="3"/>' in pyramid.dzi_manifest(3, 5, 16, 0)
    for t, o in [(0, 0), (-1, 0), (4, -1), (4, 4), (4, 5), (1, 1)]:
        with pytest.raises(ValueError):
            pyramid.dzi_plan(10, 10, t, o)
        with pytest.raises(ValueError):
            pyramid.dzi_manifest(10, 10, t, o)
    for h, w in [(0, 5), (5, 0), (-1, 3)]:
        with pytest.raises(ValueError):
            pyramid.dzi_plan(h, w)


def test_render_pyramid_refuses_before_any_device_work(tmp_path):
    from tests.test_render_many_host import _Enc, _cpu_model, _error
    tiled = dict(tile=32, tile_overlap=8, tile_any_scale=True)
    model = _cpu_model(dict(tiled))
    enc = _Enc(32)                                               # LR 40 x 56 on the host: device work would raise CiaoSRHipError
    h, w = enc.x.shape[-2:]
    assert 'smaller than the LR' in _error(lambda: model.render_pyramid(enc, scale=0.5))
    assert 'smaller than the LR' in _error(lambda: model.render_pyramid(enc, size=(h, w - 1)))
    assert 'exactly one' in _error(lambda: model.render_pyramid(enc))
    assert 'exactly one' in _error(lambda: model.render_pyramid(enc, size=(2 * h, 2 * w), scale=2))
    assert 'empty' in _error(lambda: model.render_pyramid(enc, size=(0, 4)))
    batch = _Enc(32)
    batch.x = torch.zeros(2, 3, h, w)
    assert 'one image' in _error(lambda: model.render_pyramid(batch, scale=2))
    strict = _cpu_model(dict(scale=2, tile=32, tile_overlap=8))
    assert 'tile_any_scale' in _error(lambda: strict.render_pyramid(_Enc(32), scale=2))
    # write_dzi checks its tiling before it renders
    for t, o in [(0, 0), (4, 4), (4, -1)]:
        with pytest.raises(ValueError):
            pyramid.write_dzi(model, enc, str(tmp_path / 'never'), 'x', scale=2, tile_size=t, overlap=o)
    assert not (tmp_path / 'never').exists()
    # the plan: levels of the top size, the model levels are those that cover the LR image
    from ciaosr_amd import scene_render
    sizes, first = scene_render.plan_pyramid(model, enc, scale=4)
    assert sizes == pyramid.level_sizes(4 * h, 4 * w) and sizes[-1] == (4 * h, 4 * w)
    assert [s for s in sizes if s[0] >= h and s[1] >= w] == sizes[first:] and len(sizes) - first == 3
    assert scene_render.plan_pyramid(model, enc, scale=1) == (pyramid.level_sizes(h, w), len(pyramid.level_sizes(h, w)) - 1)


def test_cli_flags_reach_write_dzi(monkeypatch, tmp_path):
    from tools import render
    base = [CONFIG, 'None', 'x.png', '--out', 'o']
    args = render.parse_args(base + ['--scale', '2'])
    assert args.dzi is None and args.dzi_tile == 254 and args.dzi_overlap == 1
    args = render.parse_args(base + ['--dzi', '4', '--dzi-tile', '16', '--dzi-overlap', '2'])           # --dzi alone is enough
    assert args.dzi == 4.0 and args.dzi_tile == 16 and args.dzi_overlap == 2 and args.scale == [] and args.view == []
    with pytest.raises(SystemExit):
        render.parse_args(base)
    # main(): the flags reach write_dzi, and the encode is planned for the pyramid's scale
    import ciaosr_amd
    import ciaosr_amd.imageio
    calls = {}

    class _Model:
        def to(self, dev):
            return self

        def eval(self):
            return self

        def gpu_png(self):
            return False

        def encode(self, lq, max_scale=None):
            calls['max_scale'] = max_scale
            return 'enc'

        def render_many(self, enc, targets, as_u8=False):
            calls['targets'] = len(targets)
            return [torch.zeros(1, 3, 4, 4) for _ in targets]

    def write_dzi(model, enc, out_dir, name, **kw):
        calls['dzi'] = (enc, out_dir, name, kw)
        return dict(levels=[(1, 1), (2, 2)], model_levels=[1], files=3, bytes=99)

    monkeypatch.setattr(ciaosr_amd, 'build_model', lambda *a, **k: _Model())
    monkeypatch.setattr(ciaosr_amd.imageio, 'imread_rgb01', lambda path: torch.zeros(3, 4, 4))
    monkeypatch.setattr(ciaosr_amd.imageio, 'imwrite', lambda img, path: calls.setdefault('written', []).append(path))
    monkeypatch.setattr(pyramid, 'write_dzi', write_dzi)
    import ciaosr_amd.checkpoint
    monkeypatch.setattr(ciaosr_amd.checkpoint, 'load_checkpoint', lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 0)
    monkeypatch.setattr(torch.Tensor, 'to', lambda self, *a, **k: self)
    out = str(tmp_path / 'o')
    paths = render.main([CONFIG, 'None', 'img7.png', '--out', out, '--scale', '2', '--dzi', '4', '--dzi-tile', '16', '--dzi-overlap', '2'])
    assert calls['dzi'] == ('enc', out, 'img7', dict(scale=4.0, tile_size=16, overlap=2))
    assert calls['max_scale'] == 4.0 and calls['targets'] == 1
    assert paths == [os.path.join(out, 'img7_x2.png')] == calls['written']
    calls.clear()
    render.main([CONFIG, 'None', 'img7.png', '--out', out, '--dzi', '3'])
    assert calls['dzi'][3] == dict(scale=3.0, tile_size=254, overlap=1) and calls['max_scale'] == 3.0 and 'targets' not in calls
    calls.clear()
    render.main([CONFIG, 'None', 'img7.png', '--out', out, '--scale', '2'])
    assert 'dzi' not in calls and calls['max_scale'] == 2


def test_abi_surface():
    from ciaosr_amd import _lib
    lib = _lib.load()
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'ciaosr_hip.h')).read(), flags=re.S)
    names = ('ciaosr_png_tiles_workspace_bytes', 'ciaosr_png_tiles_capacity_bytes', 'ciaosr_png_encode_tiles_u8')
    for name in names:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(r'\b' + name + r'\s*\(', header), name
    assert [len(_lib.SIGNATURES[n][1]) for n in names] == [3, 3, 14]
    assert _lib.SIGNATURES[names[0]][0] is C.c_size_t and _lib.SIGNATURES[names[2]][0] is C.c_int

    def sizes(rects, rows=0):
        arr = (C.c_int * (4 * len(rects)))(*[v for r in rects for v in r])
        return lib.ciaosr_png_tiles_capacity_bytes(arr, len(rects), rows), lib.ciaosr_png_tiles_workspace_bytes(arr, len(rects), rows)

    # one rect: what the single call asks for, plus the table; many: at least the sum of the worst cases (all stored) and the crops
    rects = [(3, 4, 255, 255), (0, 253, 255, 256), (9, 0, 47, 93), (5, 5, 1, 1)]
    for rows in (0, 1, 3):
        worst = filtered = bands = 0
        for y0, x0, h, w in rects:
            r = lib.ciaosr_png_rows_per_band(w, rows)
            line, nb = 3 * w + 1, -(-h // r)
            worst += sum(n + 5 * -(-n // 65535) for n in [r * line] * (nb - 1) + [(h - (nb - 1) * r) * line]) + 6
            filtered += h * line
            bands += nb
            cap1, ws1 = sizes([(y0, x0, h, w)], rows)
            assert cap1 == lib.ciaosr_png_capacity_bytes(h, w, rows) and ws1 > lib.ciaosr_png_workspace_bytes(h, w, rows) - 256
        cap, ws = sizes(rects, rows)
        assert cap >= worst and ws >= filtered + bands * (2 * 260 * 4 + 64 * 4 + 24) + 20 * len(rects)
    for bad in ([(0, 0, 0, 5)], [(0, 0, 5, 0)], [(-1, 0, 5, 5)], [(0, -1, 5, 5)], [(0, 0, 65536, 2)], [(0, 0, 4, 4), (1, 1, 0, 1)]):
        assert sizes(bad) == (0, 0), bad
    arr = (C.c_int * 4)(0, 0, 4, 4)
    assert lib.ciaosr_png_tiles_capacity_bytes(arr, 0, 0) == 0 and lib.ciaosr_png_tiles_workspace_bytes(None, 1, 0) == 0
    assert lib.ciaosr_png_tiles_capacity_bytes(arr, 1, -1) == 0


def test_encode_png_tiles_checks_on_the_host():
    from ciaosr_amd import png_hip
    from ciaosr_amd._lib import CiaoSRHipError
    from tests.test_png_host import make_image
    img = make_image(7, 5, 'random')
    with pytest.raises(CiaoSRHipError):
        png_hip.encode_png_tiles(torch.from_numpy(img), [(0, 0, 2, 2)])
    with pytest.raises(CiaoSRHipError):
        png_hip.encode_png_tiles(img, [(0, 0, 2, 2)])
    assert png_hip.check_rects([(0, 0, 7, 5), (6, 4, 1, 1)], 7, 5) == [(0, 0, 7, 5), (6, 4, 1, 1)]
    for bad in ([], [(0, 0, 0, 2)], [(0, 0, 2, 0)], [(0, 0, 8, 5)], [(0, 1, 7, 5)], [(-1, 0, 2, 2)], [(0, 0, 2)], [(0, 0, 1.5, 2)]):
        with pytest.raises(ValueError):
            png_hip.check_rects(bad, 7, 5)
