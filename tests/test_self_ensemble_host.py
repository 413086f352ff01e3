"""Self-ensemble, host side (no GPU): the group laws of the eight transforms as scene.py and include/ciaosr_hip.h define them, the
window map `scene.dihedral_window`, the validation `scene.dihedral_ids`, the ABI surface and the command-line refusals."""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def t_k(x, k):
    """T_k on the last two axes: k & 1 flips the columns, then k & 2 the rows, then k & 4 transposes."""
    if k & 1:
        x = x[..., :, ::-1]
    if k & 2:
        x = x[..., ::-1, :]
    if k & 4:
        x = np.swapaxes(x, -1, -2)
    return x


def u_k(x, k):
    """The inverse: transpose if k & 4, then flip the rows if k & 2, then the columns if k & 1."""
    if k & 4:
        x = np.swapaxes(x, -1, -2)
    if k & 2:
        x = x[..., ::-1, :]
    if k & 1:
        x = x[..., :, ::-1]
    return x


def test_group_laws():
    x = np.arange(5 * 7, dtype=np.float32).reshape(5, 7)
    members = [t_k(x, k) for k in range(8)]
    assert np.array_equal(members[0], x)
    for k in range(8):
        assert members[k].shape == ((7, 5) if k & 4 else (5, 7))
        assert np.array_equal(u_k(members[k], k), x), k
    for a in range(8):
        for b in range(a + 1, 8):
            assert members[a].shape != members[b].shape or not np.array_equal(members[a], members[b]), (a, b)


def _windows(rng, ht, wt):
    """Seeded windows of an ht x wt grid, the edge cases first: 1 x 1, full width, full height, one touching each border, the whole grid."""
    fixed = [(ht // 2, wt // 2, 1, 1), (0, 0, 1, 1), (ht - 1, wt - 1, 1, 1), (ht // 3, 0, max(1, ht // 4), wt), (0, wt // 3, ht, max(1, wt // 4)),
             (0, wt // 4, max(1, ht // 2), max(1, wt // 3)), (ht - max(1, ht // 2), wt // 4, max(1, ht // 2), max(1, wt // 3)),
             (ht // 4, 0, max(1, ht // 3), max(1, wt // 2)), (ht // 4, wt - max(1, wt // 2), max(1, ht // 3), max(1, wt // 2)), None]
    for _ in range(4):
        hh, ww = int(rng.integers(1, ht + 1)), int(rng.integers(1, wt + 1))
        fixed.append((int(rng.integers(0, ht - hh + 1)), int(rng.integers(0, wt - ww + 1)), hh, ww))
    return fixed


def test_dihedral_window_commutes_with_the_crop():
    from ciaosr_amd import scene
    rng = np.random.default_rng(11)
    n = 0
    for ht, wt in ((1, 1), (5, 7), (7, 5), (12, 12), (1, 9), (9, 1), (33, 20)):
        a = rng.permutation(ht * wt).astype(np.float32).reshape(ht, wt)
        for window in _windows(rng, ht, wt):
            i0, j0, hh, ww = scene.check_window(ht, wt, window)
            want = a[i0:i0 + hh, j0:j0 + ww]
            for k in range(8):
                ht_k, wt_k, (a0, b0, hk, wk) = scene.dihedral_window(k, ht, wt, window)
                member = t_k(a, k)
                assert member.shape == (ht_k, wt_k)
                assert 0 <= a0 and a0 + hk <= ht_k and 0 <= b0 and b0 + wk <= wt_k
                assert np.array_equal(u_k(member[a0:a0 + hk, b0:b0 + wk], k), want), (ht, wt, window, k)
                n += 1
    assert n >= 8 * 36
    with pytest.raises(ValueError):
        scene.dihedral_window(5, 4, 4, (0, 0, 5, 1))


def test_dihedral_ids():
    from ciaosr_amd import scene
    assert scene.dihedral_ids(True) == (0, 1, 2, 3, 4, 5, 6, 7)
    assert scene.dihedral_ids(None) is None and scene.dihedral_ids(False) is None
    assert scene.dihedral_ids([3, 4, 0]) == (3, 4, 0)
    assert scene.dihedral_ids((7,)) == (7,)
    assert scene.dihedral_ids(np.array([2, 1])) == (2, 1)
    for bad in ([1, 1], [0, 3, 0], 8, [8], -1, [-1], 'all', '01', 1.5, [1.5], [], [True], 0):
        with pytest.raises(ValueError):
            scene.dihedral_ids(bad)


def test_restorer_validates_before_any_device_work():
    """A bad `self_ensemble` is a ValueError although the tensors are on the host (which the device path would refuse with another error)."""
    import torch
    from tests.test_host_logic import _small_restorer
    model = _small_restorer(dict(scale=2))
    assert model.ensemble_ids() is None and model.ensemble_ids(True) == tuple(range(8))
    lq, coord, cell = torch.rand(1, 3, 8, 8), torch.zeros(1, 256, 2), torch.ones(1, 256, 2)
    for bad in ([1, 1], 'all', 8, 1.5):
        with pytest.raises(ValueError):
            model.restore(lq, coord, cell, self_ensemble=bad)
        with pytest.raises(ValueError):
            model.encode(lq, self_ensemble=bad)
    model.test_cfg = dict(scale=2, self_ensemble=[0, 5])
    assert model.ensemble_ids() == (0, 5) and model.ensemble_ids(False) is None
    with pytest.raises(ValueError):
        model.graphed_restore(lq, coord, cell)
    with pytest.raises(ValueError):
        model.encode_rgba(torch.rand(1, 4, 8, 8))
    from ciaosr_amd import tile_shard
    with pytest.raises(ValueError):
        tile_shard.clip_test_distributed(model, lq, rank=0, world=2)
    with pytest.raises(ValueError):
        tile_shard.predict_query_sharded(model, lq, coord, cell, rank=0, world=2)
    from ciaosr_amd._lib import CiaoSRHipError
    with pytest.raises(CiaoSRHipError):                                      # no CPU fallback for the transforms either
        model.restore(lq, coord, cell)


def test_ensemble_record_refusals_need_no_device():
    from ciaosr_amd import scene
    from tests.test_host_logic import _small_restorer
    model = _small_restorer(dict(scale=2))
    enc = scene.EnsembleEncoded((0, 4), [None, None], (8, 12))
    assert enc.shape == (8, 12) and enc.ids == (0, 4)
    view = scene.View(scene.view_matrix((4, 6), 2.0, 30.0, (8, 8)), (8, 8))
    for call in (lambda: model.render_view(enc, view.matrix, view.size),
                 lambda: model.render_many(enc, [scene.Grid(scale=2), view]),
                 lambda: model.render_pyramid(enc, scale=2),
                 lambda: model.prefetch(enc, [scene.Grid(scale=2)]),
                 lambda: model.render(enc, scale=2, window=(0, 0, 17, 1)),     # render's own window check, before any member is touched
                 lambda: model.render_many(enc, [])):
        with pytest.raises(ValueError):
            call()


def test_header_declares_and_lib_binds_both_entries():
    from ciaosr_amd import _lib, hip_ops
    header = open(os.path.join(REPO, 'include', 'ciaosr_hip.h')).read()
    for name in ('ciaosr_dihedral_f32', 'ciaosr_dihedral_accum_f32'):
        assert re.search(r'^int ' + name + r'\(', header, flags=re.M), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['ciaosr_dihedral_f32'][1]) == 7 and len(_lib.SIGNATURES['ciaosr_dihedral_accum_f32'][1]) == 9
    assert callable(hip_ops.dihedral) and callable(hip_ops.dihedral_accum)
    import torch
    with pytest.raises(_lib.CiaoSRHipError):                                 # a host tensor raises: no CPU fallback
        hip_ops.dihedral(torch.zeros(1, 3, 4), 1)
    with pytest.raises(_lib.CiaoSRHipError):
        hip_ops.dihedral_accum(torch.zeros(1, 3, 4), torch.zeros(1, 4, 3), 4, True)
    assert 'dihedral_ops.hip' in open(os.path.join(REPO, 'ciaosr_amd', 'csrc', 'Makefile')).read()
    assert 'ciaosr_dihedral_accum_f32' in open(os.path.join(REPO, 'INTEGRATION.md')).read()


@pytest.mark.parametrize('extra', [['--view', '10', '10', '2', '0', '--size', '8', '8'], ['--dzi', '2'], ['--alpha']])
def test_render_tool_refuses_the_flag_with_views_pyramids_and_alpha(extra, capsys):
    """argparse's error (exit status 2) from `parse_args`: no config is read and no model is built."""
    from tools import render
    base = ['cfg.py', 'None', 'img.png', '--out', 'out', '--self-ensemble']
    with pytest.raises(SystemExit) as e:
        render.parse_args(base + ['--scale', '2'] + extra)
    assert e.value.code == 2 and '--self-ensemble' in capsys.readouterr().err
    args = render.parse_args(base + ['--scale', '2', '--window', '0', '0', '4', '4'])
    assert args.self_ensemble and not render.parse_args(base[:-1] + ['--scale', '2']).self_ensemble


def test_test_tool_sets_the_key():
    from tools import test as tool
    cfg = type('Cfg', (), {})()
    cfg.test_cfg = {}
    assert 'self_ensemble' not in tool.apply_overrides(cfg, tool.parse_args(['cfg.py', 'None'])).test_cfg
    assert tool.apply_overrides(cfg, tool.parse_args(['cfg.py', 'None', '--self-ensemble'])).test_cfg['self_ensemble'] is True
