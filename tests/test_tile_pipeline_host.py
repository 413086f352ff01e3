"""CiaoSR.trunk_ahead without a GPU (`ahead=False`: the same loop on the caller's stream, no events): the order and the laziness of the
trunk calls, and that a consumer's exception between two groups leaves the generator closed with nothing pending."""
import pytest


def _pipeline(groups, calls):
    from tests.test_render_many_host import _cpu_model

    def trunk(group):
        calls.append(list(group))
        return ('patches', tuple(group)), ('feats', tuple(group))

    return _cpu_model(dict()).trunk_ahead(groups, trunk, False, None, None)


def test_groups_come_in_order_each_trunk_once_and_not_before_it_is_asked_for():
    groups, calls = [[0, 1, 2], [3]], []
    pipe = _pipeline(groups, calls)
    assert calls == []                                           # group 0's trunk is not called before group 0 is asked for
    assert next(pipe) == (('patches', (0, 1, 2)), ('feats', (0, 1, 2)))
    assert calls == [[0, 1, 2]]                                  # ... and without `ahead` group 1's not before group 1 is
    assert next(pipe) == (('patches', (3,)), ('feats', (3,)))
    assert calls == groups
    with pytest.raises(StopIteration):
        next(pipe)
    assert calls == groups                                       # once per group
    calls = []
    assert list(_pipeline(groups, calls)) == [(('patches', tuple(g)), ('feats', tuple(g))) for g in groups] and calls == groups


def test_no_groups():
    calls = []
    assert list(_pipeline([], calls)) == [] and calls == []


def test_a_consumer_exception_between_two_groups_propagates_and_closes_clean():
    import contextlib
    groups, calls = [[0, 1, 2], [3]], []
    pipe = _pipeline(groups, calls)
    with pytest.raises(KeyError, match='consumer'):
        with contextlib.closing(pipe):                           # as clip_test holds it
            for k, _ in enumerate(pipe):
                assert k == 0
                raise KeyError('consumer')
    assert calls == [[0, 1, 2]]                                  # group 1's trunk was never launched: nothing is pending
    assert pipe.gi_frame is None                                 # closed
    with pytest.raises(StopIteration):
        next(pipe)
    pipe.close()                                                 # closing again, or one never started, is clean
    fresh = _pipeline(groups, calls)
    fresh.close()
    assert calls == [[0, 1, 2]] and fresh.gi_frame is None


def test_the_generator_keeps_no_group_alive_for_its_consumer():
    import weakref

    class Maps:
        pass

    alive, refs = [], []

    def trunk(group):
        alive.append(sum(ref() is not None for ref in refs))         # earlier groups' hand-overs when this trunk is launched
        out = (Maps(), Maps())
        refs.extend(weakref.ref(m) for m in out)
        return out

    from tests.test_render_many_host import _cpu_model
    groups = [[0, 1, 2], [3], [4]]
    pipe = _cpu_model(dict()).trunk_ahead(groups, trunk, False, None, None)
    for _ in groups:                                             # as clip_test consumes it
        patches, feats = next(pipe)
        del patches, feats
    assert alive == [0, 0, 0]
