"""CPU: what the three tracking evaluators share on the host side (csrc/mot_rule.h's workspace formula behind the three
tamtr_*_workspace_bytes entry points; ops._mot_frames, the launch checks of mot_update / hota_update / trackmap_update)."""
import pytest
import torch

# Recorded from a build of the commit before the update kernels shared mot_frame_ws_bytes (553b365), by calling the three entry points
# of that library; not computed from the present formulas.  Keys are the entry point's arguments.
MOT_BYTES = {      # nq, ng, nc, gt_capacity, track_capacity
    (1, 1, 2, 8, 16): 1488, (8, 8, 2, 8, 16): 1520, (7, 9, 2, 8, 16): 1508, (64, 65, 2, 8, 16): 70448, (300, 300, 2, 8, 16): 1458016,
    (1, 1, 10, 1024, 4096): 1567056, (300, 300, 10, 1024, 4096): 1567056,
}
HOTA_BYTES = {     # nq, ng, workgroups
    (1, 1, 1): 104, (8, 8, 1): 1616, (7, 9, 1): 1608, (64, 65, 1): 71224, (300, 300, 1): 1461616,
    (1, 1, 64): 3088, (8, 8, 64): 49168, (7, 9, 64): 49168, (64, 65, 64): 2263056, (300, 300, 64): 46694416,
}
TRACKMAP_BYTES = {  # nq, ng, nc, gt_capacity, track_capacity, pair_capacity
    (1, 1, 2, 8, 16, 32): 1360, (8, 8, 2, 8, 16, 32): 1488, (7, 9, 2, 8, 16, 32): 1480, (64, 65, 2, 8, 16, 32): 70192,
    (300, 300, 2, 8, 16, 32): 1456816, (1, 1, 10, 1024, 4096, 262144): 4231280, (300, 300, 10, 1024, 4096, 262144): 4231280,
}


@pytest.mark.parametrize('entry, table', [('tamtr_mot_workspace_bytes', MOT_BYTES), ('tamtr_hota_workspace_bytes', HOTA_BYTES),
                                          ('tamtr_trackmap_workspace_bytes', TRACKMAP_BYTES)])
def test_workspace_bytes_are_those_of_the_separate_formulas(entry, table):
    from tamtr_amd import _lib
    fn = getattr(_lib.lib(), entry)
    assert {args: fn(*args) for args in table} == table


def _frames(**kw):
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)     # noqa: E731
    a = dict(tracks=torch.zeros(2, 8, 8), tcounts=i32(2), gt=torch.zeros(2, 8, 7), gcounts=i32(2))
    a.update(kw)
    return a['tracks'], a['tcounts'], a['gt'], a['gcounts']


@pytest.mark.parametrize('name, tail', [('mot_update', (2, 4, 8)), ('hota_update', (2, (4, 8, 16, 32, 8))),
                                        ('trackmap_update', (2, (4, 8, 16, 32)))])
def test_the_shared_launch_checks_name_the_called_function(name, tail):
    """Every check on the batch's rows comes before the state is looked at, so an empty state will do."""
    from tamtr_amd import TamtrHipError, ops
    fn = getattr(ops, name)
    bad = [(dict(tracks=torch.zeros(2, 8)), 'tracks'), (dict(gt=torch.zeros(2, 8, 6)), 'gt'),
           (dict(tcounts=torch.zeros(3, dtype=torch.int32)), 'tcounts'), (dict(gcounts=torch.zeros(2, dtype=torch.int64)), 'int32')]
    for kw, what in bad:
        with pytest.raises(TamtrHipError, match=what) as e:
            fn(*_frames(**kw), {}, *tail)
        assert str(e.value).startswith(name + ': '), str(e.value)
    with pytest.raises(TamtrHipError, match='iou') as e:
        fn(*_frames(), {}, *tail, iou=0)
    assert str(e.value).startswith(name + ': '), str(e.value)
