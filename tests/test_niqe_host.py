"""NIQE, host side: the float64 restatement (tests/niqe_ref.py) against the reference's own run, the eight-tap form of the halving
against MATLAB's general rule, the host finishing (`niqe_hip.features` / `finish`) against the restatement, the AGGD lookup against
`argmin`, the argument errors and the config plumbing.  Fixtures: tests/golden/niqe_cases.npz, niqe_pris_params.npz
(tools/make_niqe_golden.py, from the reference's code)."""
import os

import numpy as np
import pytest
import torch

from tests import niqe_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden')
# float64 numpy on both sides, the same operations; the window taps are added in scipy's order.  What is left is the order of the sums
# over a block (np.mean is pairwise on both sides) and scipy.special.gamma against math.gamma: measured 1.2e-15 (features), 2.1e-14 (NIQE).
REL_TOL = 1e-9


def load_cases():
    with np.load(os.path.join(GOLDEN, 'niqe_cases.npz')) as z:
        names = [str(n) for n in z['names']]
        return [dict(name=n, img=z[f'img_{i}'], crop=int(z[f'crop_{i}']), y=z[f'y_{i}'], feat32=z[f'feat32_{i}'],
                     niqe32=float(z[f'niqe32_{i}']), feat64=z[f'feat64_{i}'], niqe64=float(z[f'niqe64_{i}']),
                     g_feat=float(z['g_feat'][i]), g_niqe=float(z['g_niqe'][i])) for i, n in enumerate(names)]


@pytest.fixture(scope='module')
def cases():
    return load_cases()


@pytest.fixture(scope='module')
def params():
    from ciaosr_amd import niqe_hip
    return niqe_hip.load_params(os.path.join(GOLDEN, 'niqe_pris_params.npz'))


@pytest.fixture(scope='module')
def restated(cases, params):
    """{case name: (features, NIQE)} of the restatement on the fixture's Y planes, computed once."""
    return {c['name']: niqe_ref.niqe(c['y'], params) for c in cases}


def rel_gap(a, b):
    """Largest |a - b| / |b| over the entries that are numbers in b; the NaN patterns must agree."""
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    return float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok])))


def test_fixture_cases_are_the_ones_asked_for(cases):
    assert [c['name'] for c in cases] == ['192x288', '288x384', '96x192', '200x301_crop3', '192x288_flat']
    assert [c['img'].shape for c in cases] == [(192, 288, 3), (288, 384, 3), (96, 192, 3), (200, 301, 3), (192, 288, 3)]
    assert [c['feat64'].shape[0] for c in cases] == [6, 12, 2, 6, 6]
    nan_rows = [int(np.isnan(c['feat64']).any(axis=1).sum()) for c in cases]
    assert nan_rows == [0, 0, 0, 0, 1]
    flat = cases[4]['feat64']
    assert np.isnan(flat[2]).any() and flat[2, 0] == 0.2          # block (row 0, column 1): column-major index 2; alpha = first grid value


def test_restatement_reproduces_the_reference(cases, restated):
    for c in cases:
        feats, q = restated[c['name']]
        gf, gq = rel_gap(feats, c['feat64']), abs(q - c['niqe64']) / c['niqe64']
        print(f"{c['name']}: restatement vs reference (float64 run): features {gf:.3e}, NIQE {gq:.3e}")
        assert gf <= REL_TOL and gq <= REL_TOL


def test_eight_tap_halving_is_matlabs_general_rule():
    from ciaosr_amd import niqe_hip
    taps = np.array(niqe_hip.HALF_TAPS)
    assert taps.shape == (8,) and abs(taps.sum() - 1) == 0
    for n in range(96, 385, 2):
        w, idx = niqe_ref.matlab_resize_weights(n, 0.5)
        assert w.shape == (n // 2, 10) and idx.shape == w.shape
        assert np.abs(w[:, 0]).max() == 0 and np.abs(w[:, 9]).max() == 0          # the two outer taps of the general rule weigh nothing
        assert np.abs(w[:, 1:9] - taps[None, :]).max() <= 1e-15
        want = np.array([[niqe_hip.half_index(o, k, n) for k in range(8)] for o in range(n // 2)])
        assert np.array_equal(idx[:, 1:9], want)


def test_features_and_finish_from_numpy_moments(cases, params, restated):
    from ciaosr_amd import niqe_hip
    for c in cases:
        m = niqe_ref.moments(c['y'], params['gaussian_window'])
        feats = niqe_hip.features(m)
        want, q_want = restated[c['name']]
        assert feats.dtype == np.float64 and feats.shape == want.shape
        assert rel_gap(feats, want) <= REL_TOL
        q = niqe_hip.finish(feats, params)
        assert type(q) is float and abs(q - q_want) / q_want <= REL_TOL
        assert np.array_equal(niqe_hip.features(torch.from_numpy(m)), feats, equal_nan=True)
    # the NaN row stays in the mean and is left out of the covariance
    flat = restated['192x288_flat'][0]
    assert np.isnan(flat).any(axis=1).sum() == 1
    mu_with = np.nanmean(flat, axis=0)
    clean = flat[~np.isnan(flat).any(axis=1)]
    assert abs(mu_with[0] - clean[:, 0].mean()) > 1e-3            # alpha = 0.2 of the flat block is part of the mean
    diff = params['mu_pris_param'] - mu_with
    want = float(np.sqrt(diff @ np.linalg.pinv((params['cov_pris_param'] + np.cov(clean, rowvar=False)) / 2) @ diff.T).squeeze())
    assert abs(niqe_hip.finish(flat, params) - want) / want <= REL_TOL


def test_aggd_lookup_is_argmin():
    from ciaosr_amd import niqe_hip
    gam, r_gam = niqe_hip.gamma_tables()[:2]
    assert np.array_equal(gam, np.arange(0.2, 10.001, 0.001)) and np.abs(r_gam - niqe_ref.r_gam()).max() == 0
    rng = np.random.default_rng(5)
    mid = (r_gam[:-1] + r_gam[1:]) / 2                          # ties, or as near to one as float64 has
    t = np.concatenate([rng.uniform(r_gam[0] * 0.5, r_gam[-1] * 1.2, 6000), rng.choice(r_gam, 1500), rng.choice(mid, 1500),
                        np.nextafter(rng.choice(mid, 500), 0), np.nextafter(rng.choice(mid, 488), 1),
                        [r_gam[0], r_gam[-1], 0.0, -1.0, 5.0, 1e300, -1e300, np.inf, -np.inf, np.nan, r_gam[0] - 1e-12, r_gam[-1] + 1e-12]])
    assert t.size == 10000
    with np.errstate(all='ignore'):
        want = np.array([np.argmin((r_gam - v) ** 2) for v in t])
    got = niqe_hip.aggd_index(t)
    assert np.array_equal(got, want)
    assert got.min() == 0 and got.max() == r_gam.size - 1
    assert np.array_equal(niqe_hip.aggd_index(t.reshape(100, 100)), want.reshape(100, 100))


def test_value_errors(params):
    from ciaosr_amd import niqe_hip
    good = {k: params[k] for k in niqe_hip.PARAM_SHAPES}
    assert niqe_hip.load_params(good)['mu_pris_param'].shape == (1, 36)
    bad = [dict(good, mu_pris_param=good['mu_pris_param'].astype(np.float32)), dict(good, mu_pris_param=good['mu_pris_param'][0]),
           dict(good, cov_pris_param=good['cov_pris_param'][:35]), dict(good, gaussian_window=np.ones((5, 5))),
           {k: v for k, v in good.items() if k != 'gaussian_window'}, dict(good, cov_pris_param=np.full((36, 36), np.nan)),
           dict(good, gaussian_window=good['gaussian_window'].tolist()), os.path.join(GOLDEN, 'no_such_file.npz'), 17]
    for b in bad:
        with pytest.raises(ValueError):
            niqe_hip.load_params(b)
    img = torch.zeros(192, 192, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        niqe_hip.niqe_u8(img, params, convert_to='gray')
    with pytest.raises(ValueError):
        niqe_hip.niqe_u8(torch.zeros(96, 96, 3, dtype=torch.uint8), params)
    with pytest.raises(ValueError):
        niqe_hip.niqe_u8(img, params, crop_border=1)               # 190x190: one block
    with pytest.raises(ValueError):
        niqe_hip.moments_u8(torch.zeros(200, 100, 3, dtype=torch.uint8), params, crop_border=3)
    with pytest.raises(ValueError):
        niqe_hip.finish(np.zeros((1, 36)), params)
    one_clean = np.full((3, 36), np.nan)
    one_clean[0] = 1.0
    with pytest.raises(ValueError):
        niqe_hip.finish(one_clean, params)
    # a host image is refused: no CPU fallback
    from ciaosr_amd._lib import CiaoSRHipError
    with pytest.raises(CiaoSRHipError):
        niqe_hip.niqe_u8(img, params)


def _restorer(test_cfg):
    from ciaosr_amd import CiaoSR, LocalImplicitSREDSR
    mk = lambda i, o: dict(type='MLPRefiner', in_dim=i, out_dim=o, hidden_list=[16, 16])
    gen = dict(type=LocalImplicitSREDSR, encoder=dict(type='EDSR', in_channels=3, out_channels=3, mid_channels=8, num_blocks=1),
               imnet_q=mk(4, 3), imnet_k=mk(64, 64), imnet_v=mk(64, 64), feat_unfold=True, eval_bsize=30000)
    return CiaoSR(generator=gen, pixel_loss=dict(type='L1Loss'), rgb_mean=(0.4488, 0.4371, 0.4040), rgb_std=(1., 1., 1.),
                  test_cfg=test_cfg).eval()


def test_config_plumbing(params, monkeypatch):
    from ciaosr_amd import metrics, niqe_hip
    g = torch.Generator().manual_seed(3)
    gt = torch.rand(1, 3, 40, 52, generator=g)
    out = (gt + 0.03 * torch.randn(1, 3, 40, 52, generator=g)).clamp(0, 1)
    model = _restorer(dict(metrics=['PSNR', 'NIQE'], crop_border=2, convert_to='y'))
    assert model.niqe_params() is None and model.needs_gt()
    with pytest.raises(KeyError):
        model.evaluate(out, gt)                                    # without niqe_params the name is unknown, as before
    # with it: NIQE is asked of the device code with the quantised output and the config's crop; the order is that of `metrics`
    seen = []

    def fake(img, p, crop_border=0, convert_to='y'):
        seen.append((img, p, crop_border, convert_to))
        return 4.25
    monkeypatch.setattr(niqe_hip, 'niqe_u8', fake)
    u8 = torch.from_numpy(metrics.tensor2img(out).copy())
    for names in (['PSNR', 'NIQE'], ['NIQE', 'SSIM', 'PSNR'], ['NIQE']):
        model = _restorer(dict(metrics=names, crop_border=2, convert_to='y', niqe_params=dict(params)))
        assert model.needs_gt() is (names != ['NIQE'])
        res = model.evaluate(out, gt if names != ['NIQE'] else None, out_img=u8)
        assert list(res) == names and res['NIQE'] == 4.25
        if 'PSNR' in names:
            assert res['PSNR'] == metrics.psnr(metrics.tensor2img(out), metrics.tensor2img(gt), 2, 'y')
        img, p, crop, conv = seen[-1]
        assert img is u8 and crop == 2 and conv == 'y' and p is model.niqe_params() and p['_niqe_params'] is True
    # the output is quantised on the device: a host output without a quantised image is refused
    from ciaosr_amd._lib import CiaoSRHipError
    with pytest.raises(CiaoSRHipError):
        model.evaluate(out, None)
    with pytest.raises(ValueError):
        _restorer(dict(metrics=['NIQE'], crop_border=0, niqe_params=dict(gaussian_window=np.ones((7, 7))))).evaluate(out, None, out_img=u8)


def test_cli_flags():
    import tools.render as render
    import tools.test as cli
    from ciaosr_amd.config import Config
    path = os.path.join(REPO, 'configs', '001_localimplicitsr_edsr_div2k_g1_c64b16_1000k_unfold_lec_mulwkv_res_nonlocal.py')
    args = cli.parse_args([path, 'None', '--niqe', 'model.npz'])
    cfg = cli.apply_overrides(Config.fromfile(path), args)
    assert cfg.test_cfg['niqe_params'] == 'model.npz' and list(cfg.test_cfg['metrics'])[-1] == 'NIQE'
    assert list(cfg.test_cfg['metrics']).count('NIQE') == 1 and 'PSNR' in cfg.test_cfg['metrics']
    cfg = cli.apply_overrides(Config.fromfile(path), cli.parse_args([path, 'None']))
    assert 'niqe_params' not in cfg.test_cfg and 'NIQE' not in cfg.test_cfg['metrics']
    assert render.parse_args(['c', 'k', 'i', '--scale', '2', '--out', 'd', '--niqe', 'model.npz']).niqe == 'model.npz'
    assert render.parse_args(['c', 'k', 'i', '--scale', '2', '--out', 'd']).niqe is None
