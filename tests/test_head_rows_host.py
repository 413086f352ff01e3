"""The rule that picks the fp32 fused decode kernel's queries per workgroup (ciaosr_head_decode_rows: a pure host function).

decode_rows = 32 or 64 is taken as asked; 0 selects by launch size: 64-query workgroups from 2048 of them on (the threshold of
head_kv_fused's own rule: the launch fills the chip's 512 resident 64-row workgroups four times over), else 32."""
from ciaosr_amd import _lib

THRESHOLD = 2047 * 64 + 1        # the first launch of 2048 workgroups of 64 queries


def _rows(asked, nq):
    return _lib.load().ciaosr_head_decode_rows(asked, nq)


def test_automatic_rule_at_its_threshold():
    assert _rows(0, THRESHOLD - 1) == 32
    assert _rows(0, THRESHOLD) == 64
    assert _rows(0, 2048 * 64) == 64


def test_automatic_rule_on_the_launches_in_use():
    assert _rows(0, 1) == 32
    assert _rows(0, 48 * 4 * 48 * 4) == 32           # C2: one 48 x 48 map at x4
    assert _rows(0, 30000) == 32                     # an eval_bsize chunk
    assert _rows(0, 768 * 768) == 64                 # the 192 x 192 tile at x4 in one launch
    assert _rows(0, 1 << 20) == 64                   # the largest fused chunk


def test_explicit_rows_hold_at_every_size():
    for nq in (1, 63, 64, 65, 30000, THRESHOLD - 1, THRESHOLD, 1 << 20):
        assert _rows(32, nq) == 32
        assert _rows(64, nq) == 64
