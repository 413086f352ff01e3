"""GPU test of what the JPEG coders' shared workspace carve (csrc/jpeg_u8.h) can break and the per-kind suites do not order: consecutive
calls of different kinds, modes and chunk sizes on the ONE cached 'jpeg' workspace slot, every call carving another layout over what the
call before left there.  Every file is held to Pillow's own file of that crop with the same options, never to an earlier output.
Run on the GPU box:  python -m pytest tests -m gpu -q
"""
import numpy as np
import pytest
import torch

from tests import grey_ref
from tests.test_grey_host import pil_jpeg_grey
from tests.test_jpeg_gpu import _dev_img
from tests.test_jpeg_host import first_difference, make_image, pil_jpeg
from tests.test_jpeg_opt_host import pil_jpeg_opt
from tests.test_jpeg_prog_host import pil_jpeg_prog

pytestmark = pytest.mark.gpu
H, W, QUALITY = 37, 53, 90
RECTS = [(0, 0, 1, 1), (0, 0, 8, 8), (3, 5, 16, 16), (5, 8, 15, 17), (0, 0, H, W)]
# in the order they run: (image, subsampling, mcus_per_chunk, flags of encode_jpeg_tiles, Pillow's file of a crop)
CALLS = [('colour', '420', 0, dict(progressive=True), lambda c: pil_jpeg_prog(c, QUALITY, '420')),
         ('colour', '444', 1, dict(), lambda c: pil_jpeg(c, QUALITY, '444')),
         ('colour', '420', 0, dict(optimize=True), lambda c: pil_jpeg_opt(c, QUALITY, '420')),
         ('grey', '444', 0, dict(), lambda c: pil_jpeg_grey(c, QUALITY)),
         ('grey', '444', 5, dict(optimize=True), lambda c: pil_jpeg_grey(c, QUALITY, optimize=True)),
         ('colour', '444', 1, dict(progressive=True), lambda c: pil_jpeg_prog(c, QUALITY, '444'))]


def test_kinds_in_turn_on_one_workspace_slot():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd.jpeg_hip import encode_jpeg_tiles
    dev = torch.device('cuda:0')
    rgb = make_image(H, W, 'noise')
    host = dict(colour=rgb, grey=grey_ref.grey_of_bgr(rgb[:, :, ::-1]))
    assert host['grey'].shape == (H, W) and host['grey'].dtype == np.uint8
    imgs = dict(colour=_dev_img(rgb, 'bgr', dev), grey=torch.from_numpy(np.ascontiguousarray(host['grey'])).to(dev))
    first = None
    for k, (which, subsampling, mcus, flags, pillow) in enumerate(CALLS + CALLS[:1]):
        got = encode_jpeg_tiles(imgs[which], RECTS, quality=QUALITY, subsampling=subsampling, mcus_per_chunk=mcus, **flags)
        assert len(got) == len(RECTS)
        for (y0, x0, h, w), file in zip(RECTS, got):
            want = pillow(host[which][y0:y0 + h, x0:x0 + w])
            assert file == want, (k, which, subsampling, mcus, flags, (y0, x0, h, w), first_difference(file, want), len(file), len(want))
        if k == 0:
            first = got
    assert got == first                                       # the first call once more, over what the five others left
