"""The device PNG coder writes the bytes it wrote before its drivers, workspace layouts and packer helpers were unified:
tests/golden/png_parent_digests.json holds the length and SHA-256 of every output of `tools.make_png_parent_golden.digest_cases` as
the library of the commit before that change (version 330) wrote it on the MI355X.  The cases: RGB and RGBA in both channel orders,
`matches` off and on; a 23x31 image with default bands and with three rows per band (many bands, a short last one); a 64x200 image
whose lower half is one colour, in one band and in bands of four parse chunks with a shorter last band; 150x150 noise in one band above
65535 bytes (two stored blocks); the tiles of `RECTS` (a 1x1 tile, overlapping rects, the `chunk_first` path); `deflate_huff` on
explicit bands that do not start at 0, without matches, with the near distances only and with a scanline.
Run on the GPU box:  python -m pytest tests/test_png_refactor_gpu.py -m gpu -q
"""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def coded():
    if not torch.cuda.is_available():
        pytest.skip('GPU tests need the MI355X (run them with: python -m pytest tests -m gpu)')
    from ciaosr_amd import _lib
    from tools.make_png_parent_golden import digest_cases
    _lib.load()
    return list(digest_cases(torch.device('cuda:0')))


def test_every_output_is_the_parents(coded):
    from tools.make_png_parent_golden import digest
    with open(os.path.join(REPO, 'tests', 'golden', 'png_parent_digests.json')) as f:
        gold = json.load(f)
    assert [name for name, _, _ in coded] == list(gold), 'the fixture no longer lists the cases of the recorder'
    assert len(gold) == 63
    wrong = [(name, gold[name], digest(parts)) for name, parts, _ in coded if digest(parts) != gold[name]]
    assert not wrong, f'{len(wrong)} of {len(gold)} outputs differ from the parent commit\'s (case, recorded, now): {wrong[:4]}'


def test_the_cases_reach_every_kind_of_band(coded):
    """A condition on the inputs: stored bands, literal-only dynamic blocks and dynamic blocks with matches all occur, and some stream
    has two neighbouring bands of different kinds (`check_band_kinds` asserts both; the recorder held the parent to the same)."""
    from tools.make_png_parent_golden import check_band_kinds
    kinds = check_band_kinds([s for _, _, streams in coded for s in streams])
    assert ['stored', 'stored'] in kinds                     # the band above 65535 bytes, in two stored blocks
