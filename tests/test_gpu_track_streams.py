"""GPU: several streams at once, one tracker per stream in one launch (tamtr_*_update_streams, tamtr_gmc_estimate_streams, the
`streams=` of ops / track.ByteTracker / track.BotSort, Predictor.track_streams, tools/track.py --streams).

The oracle is the single-stream path on the same device, which test_gpu_track.py, test_gpu_botsort.py, test_gpu_botsort_reid.py and
test_gpu_gmc.py pin to the reference: a stacked tracker must equal S separate trackers BIT FOR BIT (torch.equal on tracks and tcounts
of every image and on every state tensor at the end).  It is the same instruction stream run in independent workgroups, so no
tolerance applies - which is also why the ReID case may take a smaller scene than that module's: uniqueness margins protect a
comparison between two implementations, not one between two launches of the same code.  Where a stream is also held against a numpy
twin (the ragged ByteTrack case and the end-to-end run) the bounds are test_gpu_track.py's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import bytetrack_np as T
import botsort_np as BS
import botsort_reid_np as R
import gmc_np as G
from test_botsort_host import CFG as BCFG
from test_botsort_reid_host import REID
from test_gpu_track import CFG, same_rows, same_table

pytestmark = pytest.mark.gpu
RULE = {k: v for k, v in CFG.items() if k != 'track_buffer'}


def batches(streams, F, nq, tail=(6,), dtype=np.float32):
    """S lists of per-frame rows [n, *tail] -> per launch (rows [F * S, nq, *tail], counts [F * S], active [F * S]), frame-major; a stream
    without a frame at a position keeps its image, empty."""
    S = len(streams)
    for k in range(0, max(len(s) for s in streams), F):
        rows, cnt, act = np.zeros((F * S, nq) + tail, dtype), np.zeros(F * S, np.int32), np.zeros(F * S, bool)
        for i in range(F * S):
            n, s = k + i // S, i % S
            if n < len(streams[s]):
                rows[i, :len(streams[s][n])], cnt[i], act[i] = streams[s][n], len(streams[s][n]), True
        yield rows, cnt, act


def per_image(streams, F, per_frame):
    """S lists of one array per frame (e.g. a warp) -> per launch [F * S, ...]; a position without a frame gets `far`, values that
    would show if they were ever applied."""
    S = len(streams)
    far = np.full(np.shape(per_frame[0][0]), 1e3)
    for k in range(0, max(len(s) for s in streams), F):
        yield np.stack([per_frame[i % S][k + i // S] if k + i // S < len(streams[i % S]) else far for i in range(F * S)])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_stack(trk, streams, F, nq, warps=None, feats=None, start=0, stop=None):
    """Launches start .. stop-1 of the stacked run -> per stream, per frame (tracks [nq, 8], tcount) as CPU tensors."""
    S = len(streams)
    got = [[] for _ in streams]
    wb = list(per_image(streams, F, warps)) if warps is not None else None
    fb = [b[0] for b in batches(feats, F, nq, (feats[0][0].shape[1],))] if feats is not None else None
    for k, (rows, cnt, act) in enumerate(batches(streams, F, nq)):
        if k < start or (stop is not None and k >= stop):
            continue
        kw = {**({'warps': dev(wb[k])} if wb else {}), **({'feats': dev(fb[k])} if fb else {})}
        tracks, tc = trk.update(dev(rows), dev(cnt), **kw)
        tracks, tc = tracks.cpu(), tc.cpu()
        for i in range(F * S):
            if act[i]:
                got[i % S].append((tracks[i], tc[i]))
            else:
                assert not tracks[i].any() and tc[i] == 0, 'an image without a frame left rows'
    return got


def run_single(trk, frames, F, nq, warps=None, feats=None):
    """One stream alone through a single tracker, F frames per launch -> per frame (tracks [nq, 8], tcount)."""
    got = []
    for i in range(0, len(frames), F):
        rows, cnt, _ = next(batches([frames[i:i + F]], len(frames[i:i + F]), nq))
        kw = {**({'warps': dev(np.stack(warps[i:i + F]))} if warps is not None else {}),
              **({'feats': dev(next(batches([feats[i:i + F]], len(feats[i:i + F]), nq, (feats[0].shape[1],)))[0])} if feats is not None else {})}
        tracks, tc = trk.update(dev(rows), dev(cnt), **kw)
        got += list(zip(tracks.cpu(), tc.cpu()))
    return got


def same_bits(got, want, what):
    assert len(got) == len(want), f'{what}: {len(got)} frames against {len(want)}'
    for f, ((a, na), (b, nb)) in enumerate(zip(got, want)):
        assert torch.equal(na, nb) and torch.equal(a, b), f'{what} frame {f}: rows differ from the single-stream run'


def same_state(stack, s, single, what):
    for k, v in single.state.items():
        assert torch.equal(stack.state[k][s], v), f'{what}: state[{k!r}] of stream {s} differs from the single-stream run'


# ------------------------------------------------------------------------------------------------ 1. ByteTrack, ragged streams
def ragged():
    cut = {201: 40, 203: 27, 206: 14}
    return [T.make_scene(seed, n_obj=12, frames=40, fp_every=3, gaps=[(0, 5, 3), (1, 8, 25), (2, 12, 6)])[:n] for seed, n in cut.items()]


@pytest.mark.parametrize('F', [1, 2])
def test_bytetrack_ragged_streams_equal_three_trackers_fed_alone(F):
    """S = 3, 40 / 27 / 14 frames; with F = 2 the 27-frame stream ends in the middle of a batch."""
    from tamtr_amd.track import ByteTracker
    streams = ragged()
    kw = dict(capacity=64, nq=64, **{**CFG, 'track_buffer': 10})
    stack = ByteTracker('cuda', streams=3, **kw)
    got = run_stack(stack, streams, F, 64)
    assert [len(g) for g in got] == [40, 27, 14] and sum(int(n) for g in got for _, n in g) > 300
    for s, frames in enumerate(streams):
        one = ByteTracker('cuda', **kw)
        same_bits(got[s], run_single(one, frames, F, 64), f'F {F} stream {s}')
        same_state(stack, s, one, f'F {F}')
    assert stack.state_dict()['hdr'][:, 0].tolist() == [40, 27, 14]      # every tracker counted its own frames
    # and one stream against the numpy twin directly, as test_gpu_track.against_twin does
    s = 1
    twin = T.ByteTrackNp(capacity=64, want_margin=True, **{**CFG, 'track_buffer': 10})
    for f, fr in enumerate(streams[s]):
        want = twin.update(fr)
        rows = got[s][f][0][:int(got[s][f][1])].numpy()
        same_rows(rows, fr, want[:, :4], want[:, 4].astype(int), want[:, 7].astype(int), f'stream {s} frame {f}')
    same_table({k: v[s] for k, v in stack.state_dict().items()}, twin, f'stream {s}')
    assert twin.margin > 1e-6 and twin.thr_margin > 1e-4, (twin.margin, twin.thr_margin)


# ------------------------------------------------------------------------------------------------ 2. BoT-SORT, the caller's warps
def test_botsort_reads_each_images_own_warp():
    """S = 3, F = 2, a different non-identity warp per image (and a wild one where a stream has no frame): a warp read at the wrong
    index moves a track by pixels."""
    from tamtr_amd.track import BotSort
    lens, streams, warps = (12, 9, 7), [], []
    for s, n in enumerate(lens):
        w = BS.camera_path(31 + s, n, pan=(3.0 + 2 * s, -1.5 * (s + 1)), aniso=0.002, jumps={5: (25.0 - 20 * s, 12.0)})
        w[0] = G.similarity(1.0 + s, -2.0, 0.1)      # camera_path starts with the identity; a first frame has no track to move
        streams.append(BS.through_camera(T.make_scene(301 + s, n_obj=8, frames=n, fp_every=4), w))
        warps.append(list(w))
    flat = [x for w in warps for x in w]
    assert not any(np.array_equal(x, G.IDENTITY) for x in flat) and len({x.tobytes() for x in flat}) == sum(lens)
    kw = dict(capacity=64, nq=32, gmc_method='none', **BCFG)
    stack = BotSort('cuda', streams=3, **kw)
    got = run_stack(stack, streams, 2, 32, warps=warps)
    assert sum(int(n) for g in got for _, n in g) > 100
    for s, frames in enumerate(streams):
        one = BotSort('cuda', **kw)
        same_bits(got[s], run_single(one, frames, 2, 32, warps=warps[s]), f'stream {s}')
        same_state(stack, s, one, 'botsort')
    blind = BotSort('cuda', **kw)      # the warps do matter here: without them stream 0's rows come out different
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(got[0], run_single(blind, streams[0], 2, 32)))


# ------------------------------------------------------------------------------------------------ 3. BoT-SORT with ReID
def test_botsort_reid_streams_keep_their_own_features():
    """S = 2, F = 2, D = 8; scenes, camera and feature recipe are test_gpu_botsort_reid.fresh's, with 6 objects so that D = 8 holds
    the objects' axes (object_features needs n_obj + 1 < D)."""
    from tamtr_amd.track import BotSort
    dim, streams, warps, feats = 8, [], [], []
    for seed, n in ((402, 18), (403, 13)):
        scene, who = R.make_scene(seed, n_obj=6, frames=n, fp_every=3, gaps=[(0, 5, 3), (1, 8, 6)], empty=(9,))
        w = BS.camera_path(seed, n, pan=(4.0, -2.0), aniso=0.003, jumps={10: (30.0, -20.0)})
        streams.append(BS.through_camera(scene, w)), warps.append(list(w)), feats.append(R.object_features(seed, who, 6, dim))
    kw = dict(capacity=64, nq=32, with_reid=True, reid_dim=dim, gmc_method='none', **{**BCFG, **REID})
    stack = BotSort('cuda', streams=2, **kw)
    assert tuple(stack.state['feat'].shape) == (2, 64, dim)
    got = run_stack(stack, streams, 2, 32, warps=warps, feats=feats)
    assert sum(int(n) for g in got for _, n in g) > 60
    for s, frames in enumerate(streams):
        one = BotSort('cuda', **kw)
        same_bits(got[s], run_single(one, frames, 2, 32, warps=warps[s], feats=feats[s]), f'stream {s}')
        same_state(stack, s, one, 'reid')      # state['feat'] included
        assert one.state['feat'].abs().sum() > 0
    assert not torch.equal(stack.state['feat'][0], stack.state['feat'][1])


# ------------------------------------------------------------------------------------------------ 4. isolation
def separated(n, frames, seed):
    """n objects 150 px apart that drift a pixel a frame: every one becomes a track."""
    rng = np.random.default_rng(seed)
    base = np.stack([np.arange(n) * 150.0, np.full(n, 50.0), np.arange(n) * 150.0 + 60, np.full(n, 150.0), rng.uniform(0.7, 0.9, n), np.zeros(n)], 1)
    return [(base + np.float32([f, f, f, f, 0, 0])).astype(np.float32) for f in range(frames)]


def test_an_overflowing_stream_leaves_its_neighbour_and_the_memory_around_alone():
    """Capacity 4; stream 0 brings 8 objects, stream 1 brings 2.  Canaries after every stacked table and after the workspace."""
    from tamtr_amd import ops
    from tamtr_amd.track import ByteTracker, TrackerOverflow
    cap, nq, pad, S = 4, 32, 64, 2
    streams = [separated(8, 4, 1), separated(2, 4, 2)]
    big, state = {}, {}
    for k, dt, tail in ops.TRACK_STATE_SPEC + (('hdr', torch.int32, None),):
        rows = S * (cap if tail is not None else 8)
        big[k] = torch.full((rows + pad,) + (tail or ()), 77, dtype=dt, device='cuda')
        big[k][:rows] = 0
        state[k] = big[k][:rows].view((S, cap) + tail if tail is not None else (S, 8))
    state['hdr'][:, 1] = 1
    need = ops.bytetrack_workspace_bytes(cap, nq, S)
    ws = torch.full((need + 4096,), 77, dtype=torch.uint8, device='cuda')
    one = ByteTracker('cuda', capacity=cap, nq=nq, **CFG)
    want = run_single(one, streams[1], 2, nq)
    got = []
    for rows, cnt, _ in batches(streams, 2, nq):
        tracks, tc = ops.bytetrack_update(dev(rows), dev(cnt), state, cap, workspace=ws[:need], streams=S, **RULE)
        got += [(tracks[i].cpu(), tc[i].cpu()) for i in (1, 3)]
    torch.cuda.synchronize()
    hdr = state['hdr'].cpu().numpy()
    assert hdr[0, T.H_OVER] > 0 and hdr[1, T.H_OVER] == 0 and hdr[0, T.H_LIVE] == cap and hdr[1, T.H_LIVE] == 2
    same_bits(got, want, 'stream 1 next to an overflowing stream')
    for k, v in one.state.items():
        assert torch.equal(state[k][1], v), f'stream 1: state[{k!r}] differs from its single run'
    for k in big:
        assert bool((big[k][state[k].shape[0] * state[k].shape[1]:] == 77).all()), f'{k}: written past the stacked table'
    assert bool((ws[need:] == 77).all()), 'written past the workspace'
    with pytest.raises(TrackerOverflow, match=r'\(stream 0: \d+\)'):
        ByteTracker('cuda', capacity=cap, nq=nq, streams=S, **CFG).check_overflow(hdr[:, T.H_OVER])


def test_reset_of_one_stream():
    from tamtr_amd.track import ByteTracker
    streams = [T.make_scene(103 + s, n_obj=5, frames=8, fp_every=0, p_low=0.0) for s in range(2)]
    kw = dict(capacity=64, nq=32, **CFG)
    stack = ByteTracker('cuda', streams=2, **kw)
    head = run_stack(stack, streams, 2, 32, stop=2)
    assert stack.state_dict()['hdr'][:, 1].min() > 1
    stack.reset(stream=1)
    tail = run_stack(stack, streams, 2, 32, start=2)
    whole = ByteTracker('cuda', **kw)
    same_bits(head[0] + tail[0], run_single(whole, streams[0], 2, 32), 'stream 0 across the reset of stream 1')
    same_state(stack, 0, whole, 'reset')
    fresh = ByteTracker('cuda', **kw)
    same_bits(tail[1], run_single(fresh, streams[1][4:], 2, 32), 'stream 1 after its reset')
    same_state(stack, 1, fresh, 'reset')
    assert min(int(t[:int(n), 4].min()) for t, n in tail[1] if n) == 1      # its ids start at 1 again
    stack.reset()
    assert stack.state_dict()['hdr'].tolist() == [[0, 1, 0, 0, 0, 0, 0, 0]] * 2 and not stack.state['meta'].any()


# ------------------------------------------------------------------------------------------------ 5. resume
def test_resume_from_a_state_dict_and_a_stream_on_its_own():
    from tamtr_amd import ops
    from tamtr_amd.track import ByteTracker
    streams = [s[:12] for s in ragged()[:2]] + [ragged()[2][:7]]
    kw = dict(capacity=64, nq=64, **{**CFG, 'track_buffer': 10})
    whole = ByteTracker('cuda', streams=3, **kw)
    ref = run_stack(whole, streams, 2, 64)
    a = ByteTracker('cuda', streams=3, **kw)
    head = run_stack(a, streams, 2, 64, stop=3)
    sd = a.state_dict()
    assert sd['mean'].shape == (3, 64, 8) and sd['hdr'].shape == (3, 8)
    b = ByteTracker('cuda', streams=3, **kw)
    b.load_state_dict(sd)
    tail = run_stack(b, streams, 2, 64, start=3)
    for s in range(3):
        same_bits(head[s] + tail[s], ref[s], f'resumed stream {s}')
    for k, v in whole.state.items():
        assert torch.equal(b.state[k], v), f'state[{k!r}] after the resume'
    with pytest.raises(ValueError, match='shape'):
        ByteTracker('cuda', **kw).load_state_dict(sd)      # a stacked state is not a single tracker's
    # stream_state(s): contiguous views that the single-stream op takes as they are, and that continue stream s as the stack would
    c = ByteTracker('cuda', streams=3, **kw)
    c.load_state_dict(sd)
    s, view = 1, c.stream_state(1)
    assert all(v.is_contiguous() and v.data_ptr() == c.state[k][s].data_ptr() for k, v in view.items())
    got = []
    for i in range(6, 12, 2):
        rows, cnt, _ = next(batches([streams[s][i:i + 2]], 2, 64))
        tracks, tc = ops.bytetrack_update(dev(rows), dev(cnt), view, 64, max_time_lost=c.max_time_lost, **RULE)
        got += list(zip(tracks.cpu(), tc.cpu()))
    same_bits(got, ref[s][6:], 'stream 1 continued by the single-stream op')
    for k in view:
        assert torch.equal(c.state[k][s], whole.state[k][s]) and torch.equal(c.state[k][0], dev(sd[k][0])), k


# ------------------------------------------------------------------------------------------------ 6. the estimator
def gmc_streams(H=128):
    out = []
    for seed, mseed in ((21, 5), (22, 6)):
        frames, _ = G.make_frames(seed, 128, 5, G.random_motions(mseed, 4, max_t=8.0, S=128))
        out.append(np.ascontiguousarray(frames[:, :H]))
    return out, [[1, 1, 0, 1, 1], [1, 1, 1, 1, 1]]      # one image of stream 0, in mid-sequence, has no detections


def gmc_single(frames, counts, F, scale):
    from tamtr_amd import ops
    H, W = frames.shape[1:3]
    state, w, st = ops.gmc_state(H, W, 'cuda'), [], []
    for i in range(0, len(frames), F):
        n = len(frames[i:i + F])
        a, b = ops.gmc_estimate(dev(frames[i:i + F]), torch.tensor(counts[i:i + F], dtype=torch.int32).cuda(), np.tile(scale, (n, 1)), state)
        w.append(a.cpu()), st.append(b.cpu())
    return torch.cat(w), torch.cat(st), state


_GMC_SINGLE = {}


def gmc_singles(H, F):
    if (H, F) not in _GMC_SINGLE:
        frames, counts = gmc_streams(H)
        _GMC_SINGLE[H, F] = [gmc_single(frames[s], counts[s], F, [1.25, 0.8]) for s in range(2)]
    return _GMC_SINGLE[H, F]


@pytest.mark.parametrize('H,F', [(128, 1), (128, 2), (96, 2)])
def test_estimator_pairs_within_a_stream(H, F):
    """S = 2, five frames per stream; 96 x 128 is the non-square size.  With F = 2 the last batch holds one frame of each stream and
    two images without a frame."""
    from tamtr_amd import ops
    frames, counts = gmc_streams(H)
    S, W = 2, 128
    state = ops.gmc_state(H, W, 'cuda', streams=S)
    ws = torch.empty(ops.gmc_workspace_bytes(F * S, H, W), device='cuda', dtype=torch.uint8)
    got_w, got_s, pairs = [[], []], [[], []], [[], []]
    for k in range(0, 5, F):
        at = [(k + i // S, i % S) for i in range(F * S)]
        fr = np.stack([frames[s][n] if n < 5 else frames[0][0] for n, s in at])
        cnt = [counts[s][n] if n < 5 else 0 for n, s in at]
        warps, stats = ops.gmc_estimate(dev(fr), torch.tensor(cnt, dtype=torch.int32).cuda(), np.tile([1.25, 0.8], (F * S, 1)), state, ws, streams=S)
        pair = ops.gmc_workspace_views(ws, F * S, H, W)['pair'].cpu().tolist()
        for i, (n, s) in enumerate(at):
            if n < 5:
                got_w[s].append(warps[i].cpu()), got_s[s].append(stats[i].cpu()), pairs[s].append(pair[i])
            else:
                assert pair[i] == -2 and torch.equal(warps[i].cpu(), torch.from_numpy(G.IDENTITY)) and not stats[i].any()
    for s in range(S):
        w, st, one = gmc_singles(H, F)[s]
        assert torch.equal(torch.stack(got_w[s]), w) and torch.equal(torch.stack(got_s[s]), st), f'stream {s}: warps / stats'
        for k, v in one.items():
            assert torch.equal(state[k][s], v), f'stream {s}: state[{k!r}]'
        assert int(st[:, 3].sum()) >= 3, 'the single-stream run used too few fits to compare anything'
    # pairing: -2 nothing, -1 the stream's state, else an image of the same batch, which must be of the same stream
    if F == 1:
        assert pairs == [[-2, -1, -2, -1, -1], [-2, -1, -1, -1, -1]]      # stream 0 skips its empty frame, stream 1 does not
    else:
        assert pairs == [[-2, 0, -2, -1, -1], [-2, 1, -1, 1, -1]]      # stream 0's fourth frame passes over image 0 of its batch
    assert not torch.equal(got_w[0][3], got_w[1][3])


def test_botsort_streams_estimate_resume_and_reset():
    """BotSort(streams=2) fed frames: the estimator's stacked state rides in state_dict, and reset(stream=) forgets one stream's frame."""
    from tamtr_amd.track import BotSort
    frames, _ = gmc_streams()
    scene = [T.make_scene(301 + s, n_obj=4, frames=5, fp_every=0, p_low=0.0) for s in range(2)]
    kw = dict(capacity=32, nq=32, **BCFG)

    def step(trk, n):
        rows, cnt, _ = next(batches([scene[0][n:n + 1], scene[1][n:n + 1]], 1, 32))
        tracks, tc = trk.update(dev(rows), dev(cnt), frames=dev(np.stack([frames[0][n], frames[1][n]])))
        return tracks.cpu(), tc.cpu(), trk.last_warps.cpu()

    whole = BotSort('cuda', streams=2, **kw)
    ref = [step(whole, n) for n in range(4)]
    a = BotSort('cuda', streams=2, **kw)
    [step(a, n) for n in range(2)]
    sd = a.state_dict()
    assert sd['gmc_pyr'].shape[0] == 2 and sd['gmc_hdr'].shape == (2, 4) and sd['gmc_hdr'][:, 0].tolist() == [1, 1]
    b = BotSort('cuda', streams=2, **kw)
    b.load_state_dict(sd)
    for n in (2, 3):
        assert all(torch.equal(x, y) for x, y in zip(step(b, n), ref[n])), f'frame {n} after the resume'
    assert all(torch.equal(b.gmc[k], whole.gmc[k]) for k in b.gmc) and all(torch.equal(b.state[k], whole.state[k]) for k in b.state)
    assert not torch.equal(ref[3][2][0], torch.from_numpy(G.IDENTITY)) and not torch.equal(ref[3][2][1], torch.from_numpy(G.IDENTITY))
    b.reset(stream=0)
    _, _, w = step(b, 4)
    assert torch.equal(w[0], torch.from_numpy(G.IDENTITY)) and not torch.equal(w[1], torch.from_numpy(G.IDENTITY))
    assert b.state_dict()['hdr'][:, 0].tolist() == [1, 5]


# ------------------------------------------------------------------------------------------------ 7. argument checks
def test_argument_checks_come_before_any_launch():
    """Every refusal leaves the tables as they were: nothing was launched."""
    from tamtr_amd import TamtrHipError, ops
    from tamtr_amd.track import ByteTracker
    trk = ByteTracker('cuda', capacity=16, nq=32, streams=2, **CFG)
    before = {k: v.clone() for k, v in trk.state.items()}
    out, cnt = torch.rand(3, 32, 6, device='cuda'), torch.full((3,), 5, dtype=torch.int32, device='cuda')
    with pytest.raises(TamtrHipError, match='no multiple of streams = 2'):
        trk.update(out, cnt)
    out, cnt = torch.rand(4, 32, 6, device='cuda'), torch.full((4,), 5, dtype=torch.int32, device='cuda')
    with pytest.raises(TamtrHipError, match=r"state\['mean'\]"):      # state without the leading S
        ops.bytetrack_update(out, cnt, trk.stream_state(0), 16, streams=2)
    small = torch.empty(ops.bytetrack_workspace_bytes(16, 32), device='cuda', dtype=torch.uint8)
    with pytest.raises(TamtrHipError, match='workspace must be'):      # a workspace sized for one tracker
        ops.bytetrack_update(out, cnt, trk.state, 16, workspace=small, streams=2)
    with pytest.raises(TamtrHipError, match='warps must be'):
        ops.botsort_update(out, cnt, trk.state, 16, torch.zeros(2, 2, 3, dtype=torch.float64, device='cuda'), streams=2)
    fr = torch.zeros(3, 64, 64, 3, dtype=torch.uint8, device='cuda')
    with pytest.raises(TamtrHipError, match='no multiple of streams = 2'):
        ops.gmc_estimate(fr, cnt[:3], np.ones((3, 2)), ops.gmc_state(64, 64, 'cuda', streams=2), streams=2)
    with pytest.raises(TamtrHipError, match=r"state\['pyr'\]"):
        ops.gmc_estimate(fr[:2], cnt[:2], np.ones((2, 2)), ops.gmc_state(64, 64, 'cuda'), streams=2)
    torch.cuda.synchronize()
    assert all(torch.equal(trk.state[k], v) for k, v in before.items())


# ------------------------------------------------------------------------------------------------ 8. end to end
def test_predictor_track_streams_end_to_end(tmp_path):
    """Two directories of 3 and 2 images, two frames per stream and batch: this run's own detections, de-interleaved, replayed through
    one numpy twin per stream (the bounds and the margin precondition of test_predictor_track_end_to_end)."""
    from test_gpu_predict import CONF, IMGSZ, NC, _images, _model, _text_feats
    from tamtr_amd.predict import Predictor
    from tamtr_amd.track import ByteTracker
    src = _images(tmp_path)
    names = {i: f'c{i}' for i in range(NC)}
    pred = Predictor(_model().cuda(), names, _text_feats(), imgsz=IMGSZ, conf=CONF, iou=0.7, batch=2, dtype='fp32')
    plain = list(pred.predict(str(src)))
    scores = np.sort(np.concatenate([d.conf.numpy() for d in plain]))
    kw = dict(track_high_thresh=float(scores[len(scores) // 2]) * 1.0001, track_low_thresh=float(scores[len(scores) // 8]) * 1.0001,
              new_track_thresh=float(scores[len(scores) * 3 // 4]) * 1.0001, match_thresh=0.8, track_buffer=30)
    files = sorted(str(p) for p in src.iterdir())
    for s, group in enumerate((files[:3], files[3:])):
        (tmp_path / f'cam{s}').mkdir()
        for f in group:
            os.rename(f, tmp_path / f'cam{s}' / os.path.basename(f))
    sources = [str(tmp_path / 'cam0'), str(tmp_path / 'cam1')]
    with pytest.raises(ValueError, match='streams=2'):
        pred.track_streams(sources, tracker=ByteTracker('cuda', capacity=256, nq=300, **kw))
    trk = ByteTracker('cuda', capacity=256, nq=300, streams=2, **kw)
    calls, run_batch = [], pred.run_batch

    def spy(ims, tracker=None, **more):      # this run's own detections, as they left the device
        calls.append((run_batch(ims, tracker, **more), more['active']))
        return calls[-1][0]

    pred.run_batch = spy
    seen0 = pred.seen
    got = [[], []]
    for s, det in pred.track_streams(sources, tracker=trk, frames_per_stream=2):
        got[s].append(det)
    assert [[os.path.basename(d.path) for d in g] for g in got] == [['im0.png', 'im1.png', 'im2.png'], ['im3.png', 'im4.png']]
    assert [a for _, a in calls] == [[True] * 4, [True, False, False, False]] and pred.seen - seen0 == 5      # one forward per batch of 4
    dets = [[], []]
    for res, active in calls:
        assert res[0].shape[0] == 4 and all(int(res[2][i]) == 0 and int(res[4][i]) == 0 for i in range(4) if not active[i])
        for i in range(4):
            if active[i]:
                dets[i % 2].append(res[0][i, :int(res[2][i])].numpy())
    n_ids = 0
    for s in range(2):
        twin = T.ByteTrackNp(capacity=256, want_margin=True, **kw)
        for f, (det, raw) in enumerate(zip(got[s], dets[s])):
            want = twin.update(raw)
            if len(want) == 0:
                assert det.id is None and np.array_equal(det.boxes.numpy(), raw), f'stream {s} frame {f}'
                continue
            order, worder = np.argsort(det.id.numpy()), np.argsort(want[:, 4])
            assert np.array_equal(det.id.numpy()[order], want[worder, 4].astype(np.int64)), f'stream {s} frame {f}: ids'
            idx = want[worder, 7].astype(int)
            assert np.array_equal(det.boxes.numpy()[order, 4:6], raw[idx, 4:6]), f'stream {s} frame {f}: score / cls of detection idx'
            np.testing.assert_allclose(det.boxes.numpy()[order, :4], want[worder, :4], rtol=1e-6, atol=5e-4)
            n_ids += len(want)
        print('stream', s, 'twin margin', twin.margin, 'threshold margin', twin.thr_margin)
        assert twin.margin > 1e-6, 'precondition: this run has an assignment that is not unique'
        assert min(int(d.id.min()) for d in got[s] if d.id is not None) == 1      # every stream's ids start at 1
    assert n_ids > 0 and pred.speed()['track'] > 0 and set(pred.speed()) == {'load', 'h2d', 'forward', 'postprocess', 'track', 'd2h'}


def test_track_cli_streams_runs_in_a_child_process(tmp_path):
    """tools/track.py --streams 2 on two sequence directories of 3 and 2 frames: one MOT file per sequence, ids start at 1 in each."""
    from PIL import Image
    from test_gpu_predict import CONF, IMGSZ, NC, _model, _text_feats
    rng = np.random.default_rng(4)
    for seq, n in (('uav1', 3), ('uav2', 2)):
        (tmp_path / 'sequences' / seq).mkdir(parents=True)
        for i in range(n):
            Image.fromarray(rng.integers(0, 256, (96, 128, 3), dtype=np.uint8)).save(tmp_path / 'sequences' / seq / f'{i + 1:07d}.png')
    sd = _model().state_dict()
    torch.save({'model': sd, 'ema': sd}, tmp_path / 'best.pt')
    names = [f'c{i}' for i in range(NC)]
    np.savez(tmp_path / 'feats.npz', texts=np.array(names), feats=_text_feats().numpy())
    (tmp_path / 'bytetrack.yaml').write_text('tracker_type: bytetrack\ntrack_high_thresh: 0.00004\ntrack_low_thresh: 0.00002\n'
                                             'new_track_thresh: 0.00005\ntrack_buffer: 30\nmatch_thresh: 0.8\n')
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'track.py'), '--weights', str(tmp_path / 'best.pt'), '--text-feats', str(tmp_path / 'feats.npz'),
           '--names', ','.join(names), '--source', str(tmp_path / 'sequences'), '--tracker', str(tmp_path / 'bytetrack.yaml'), '--imgsz', str(IMGSZ),
           '--batch', '2', '--streams', '2', '--conf', str(CONF), '--save-txt', '--save-conf', '--save-mot', '--project', str(tmp_path / 'runs'),
           '--name', 'TAMTR', '--dtype', 'fp32', '--capacity', '512']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    out = tmp_path / 'runs' / 'TAMTR'
    assert res['sequences'] == 2 and res['images'] == 5 and res['streams'] == 2 and res['track_rows'] > 0 and res['save_dir'] == str(out)
    total = 0
    for seq, n in (('uav1', 3), ('uav2', 2)):
        mot = [ln.split(',') for ln in (out / f'{seq}.txt').read_text().splitlines()]
        assert mot and all(len(ln) == 10 and ln[8:] == ['-1', '-1'] for ln in mot)
        assert mot[0][0] == '1' and max(int(ln[0]) for ln in mot) <= n and min(int(ln[1]) for ln in mot) == 1
        first = np.loadtxt(out / 'labels' / seq / '0000001.txt', ndmin=2)
        assert first.shape[1] == 7 and sorted(first[:, 6].astype(int)) == sorted(int(ln[1]) for ln in mot if ln[0] == '1')
        total += len(mot)
    assert total == res['track_rows']
