"""GPU: tamtr_gmc_estimate (csrc/gmc.hip) against its numpy statement (tests/gmc_np.py) and against synthetic ground truth, stage by
stage and end to end through BotSort and Predictor.track.

What must be equal: grey, every pyramid level, the keypoint slots and the counts (integer arithmetic, fp32 op by op), the pairing, the
fit's chosen hypothesis and inlier mask.  What is bounded: LK runs in fp32 and sums its 441 terms in another order than numpy, so its
positions are held to four times the distance between the twin's own fp32 and fp64 runs on the same input, measured at run time; the
fit repeats the twin's fp64 operations, and its warp is held to 1e-9 relative.  Warps meet the half-pixel corner condition of
tests/test_gmc_host.py."""
import numpy as np
import pytest
import torch

import gmc_np as G
from test_gmc_host import case

pytestmark = pytest.mark.gpu


def estimate(frames, counts, state=None, scale=None, stages=15, ws=None):
    from tamtr_amd import ops
    B, H, W, _ = frames.shape
    state = ops.gmc_state(H, W, 'cuda') if state is None else state
    ws = torch.empty(ops.gmc_workspace_bytes(B, H, W), device='cuda', dtype=torch.uint8) if ws is None else ws
    scale = np.ones((B, 2)) if scale is None else scale
    warps, stats = ops.gmc_estimate(torch.from_numpy(np.ascontiguousarray(frames)).cuda(), torch.tensor(counts, dtype=torch.int32).cuda(), scale,
                                    state, ws, stages)
    return warps.cpu().numpy(), stats.cpu().numpy(), state, {k: v.cpu().numpy() for k, v in ops.gmc_workspace_views(ws, B, H, W).items()}


def levels(flat, H, W):
    from tamtr_amd import ops
    return [flat[o:o + h * w].reshape(h, w) for h, w, o in ops.gmc_levels(H, W)]


@pytest.mark.parametrize('S,movers,seed', [(128, 0, 3), (256, 2, 2)])
def test_integer_stages_equal_the_twin_and_lk_is_within_its_bound(S, movers, seed):
    frames = case(S, movers, seed)[0][:2]
    _, stats, _, v = estimate(frames, [1, 1])
    pyrs = [G.pyramid(G.grey(f)) for f in frames]
    kps = [G.keypoints(G.corner_response(p[0])) for p in pyrs]
    for b in range(2):
        got = levels(v['pyr'][b], S, S)
        assert len(got) == len(pyrs[b]) == G.n_levels(S, S)
        for l, (a, w) in enumerate(zip(got, pyrs[b])):
            assert np.array_equal(a, w), f'frame {b} level {l}'
        assert np.array_equal(v['kp'][b], kps[b]), f'frame {b}: keypoint slots'
    assert v['pair'].tolist() == [-2, 0] and stats[1, 0] == (kps[0] >= 0).sum() and not stats[0].any()
    # LK from frame 0's keypoints: status against the fp64 twin, positions against the twin's own fp32 / fp64 distance
    p64, s64 = G.lk(pyrs[0], pyrs[1], kps[0], np.float64)
    p32, s32 = G.lk(pyrs[0], pyrs[1], kps[0], np.float32)
    differ = int((v['status'][1] != s64).sum())
    both = (v['status'][1] == 2) & (s64 == 2) & (s32 == 2)
    bound = 4 * np.abs(p32[both].astype(np.float64) - p64[both]).max()
    err = np.abs(v['pts'][1][both].astype(np.float64) - p64[both]).max()
    print(f'S {S}: status differs on {differ} of {int((kps[0] >= 0).sum())} points, |device - twin64| {err:.3e} against the bound {bound:.3e}')
    assert differ <= 0.01 * (kps[0] >= 0).sum() and both.sum() > 200
    assert err <= bound
    assert stats[1, 1] == (v['status'][1] == 2).sum()


def test_partial_tiles_and_a_non_square_frame():
    """72 x 136: two levels, tiles of 8 rows and 8 columns at the far edges."""
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (1, 72, 136, 3), dtype=np.uint8)
    frames[0, 20:50, 30:90] = G._texture(rng, 60)[:30, :, None].astype(np.uint8)
    _, _, _, v = estimate(frames, [1])
    pyr = G.pyramid(G.grey(frames[0]))
    for l, (a, w) in enumerate(zip(levels(v['pyr'][0], 72, 136), pyr)):
        assert np.array_equal(a, w), f'level {l}'
    assert np.array_equal(v['kp'][0], G.keypoints(G.corner_response(pyr[0])))


@pytest.mark.parametrize('n', [4, 5, 64, 1024])
def test_fit_on_given_points_equals_the_twin(n):
    from tamtr_amd import ops
    rng = np.random.default_rng(n)
    M = G.similarity(4.5, -7.25, 1.5, 1.01, centre=(32, 32))
    src = rng.uniform(0, 63, (n, 2))
    dst = src @ M[:, :2].T + M[:, 2] + rng.normal(0, 0.05, (n, 2))
    bad = rng.random(n) < 0.3
    bad[:4] = False
    dst[bad] += rng.uniform(8, 30, (int(bad.sum()), 2))
    pts, status = np.zeros((G.SLOTS, 4), np.float32), np.zeros(G.SLOTS, np.int32)
    slots = np.sort(rng.choice(G.SLOTS, n, replace=False))
    pts[slots], status[slots] = np.concatenate([src, dst], 1).astype(np.float32), 2
    status[np.setdiff1d(np.arange(G.SLOTS), slots)[:10 if n < G.SLOTS else 0]] = 1      # lost points in between are passed over
    scale = np.array([[1.5, 1.25]])
    ws = torch.zeros(ops.gmc_workspace_bytes(1, 64, 64), device='cuda', dtype=torch.uint8)
    view = ops.gmc_workspace_views(ws, 1, 64, 64)
    view['pts'][0].copy_(torch.from_numpy(pts))
    view['status'][0].copy_(torch.from_numpy(status))
    view['pair'].fill_(-1)
    warp, stats, _, v = estimate(np.zeros((1, 64, 64, 3), np.uint8), [1], scale=scale, stages=8, ws=ws)
    want, (tracked, inl, used), k, mask = G.fit_pairs(pts, status, scale[0])
    assert stats[0].tolist() == [int((status > 0).sum()), tracked, inl, used] and v['fit'][0, 0] == k
    assert np.array_equal(v['fit'][0, 8:8 + n].astype(bool), mask)
    if n == 4:
        assert np.array_equal(warp[0], G.IDENTITY) and not used
        return
    assert used and not mask[bad].any()
    assert np.abs(warp[0] - want).max() <= 1e-9 * np.abs(want).max()


def test_end_to_end_batches_pairing_and_botsort():
    """Seven frames, the fourth without detections, at B = 1 and B = 3 (the sequence crosses batch boundaries): the same warps bit for
    bit, the empty frame unpaired, the next warp spanning two frames, every warp within half a pixel of the truth; then the chain
    gmc_estimate -> warps -> BotSort through update(frames=...), against update(warps=...) with the same warps."""
    from test_gpu_track import pack
    from tamtr_amd.track import BotSort
    S = 128
    frames, truth = G.make_frames(21, S, 7, G.random_motions(5, 6, max_t=8.0, S=S))
    counts = [1, 1, 1, 0, 1, 1, 1]
    scale = np.tile([[1.25, 0.8]], (7, 1))
    runs = {}
    for B in (1, 3):
        state, w, s = None, [], []
        for i in range(0, 7, B):
            a, b, state, _ = estimate(frames[i:i + B], counts[i:i + B], state, scale[i:i + B])
            w.append(a), s.append(b)
        runs[B] = np.concatenate(w), np.concatenate(s)
    assert np.array_equal(runs[1][0], runs[3][0]) and np.array_equal(runs[1][1], runs[3][1])
    w, s = runs[3]
    D, Di = np.diag([1.25, 0.8, 1.0]), np.diag([0.8, 1.25, 1.0])
    full = lambda t: np.vstack([truth[t], [0, 0, 1]])      # noqa: E731
    for t in range(7):
        if t in (0, 3):
            assert np.array_equal(w[t], G.IDENTITY) and not s[t].any()
            continue
        want = (D @ (full(4) @ full(3) if t == 4 else full(t)) @ Di)[:2]      # in original pixels; frame 4 is paired with frame 2
        err = G.corner_error(w[t], want, 0.8 * S, 1.25 * S)
        print(f'frame {t}: corner error {err:.3f} original px, stats {s[t].tolist()}')
        assert s[t, 3] == 1 and err <= 0.5
    # the tracker: estimated inside update() = handed over
    rng = np.random.default_rng(2)
    dets = [np.concatenate([rng.uniform(20, 100, (5, 2)), np.zeros((5, 2)), np.full((5, 1), 0.9), np.zeros((5, 1))], 1).astype(np.float32)
            for _ in range(3)]
    for d in dets:
        d[:, 2:4] = d[:, :2] + 20
    out, cnt = pack(dets, 32)
    a, b = BotSort('cuda', capacity=16, nq=32), BotSort('cuda', capacity=16, nq=32)
    fr = torch.from_numpy(frames[:3]).cuda()
    ra = a.update(out, cnt, frames=fr, scale=scale[:3])
    assert np.array_equal(a.last_warps.cpu().numpy(), runs[3][0][:3]) and np.array_equal(a.last_stats.cpu().numpy(), runs[3][1][:3])
    rb = b.update(out, cnt, warps=a.last_warps)
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1])
    # resume: the estimator's state travels in state_dict
    c = BotSort('cuda', capacity=16, nq=32)
    c.load_state_dict(a.state_dict())
    nxt = torch.from_numpy(frames[3:5]).cuda()
    cn = torch.tensor(counts[3:5], dtype=torch.int32).cuda()
    assert torch.equal(a.estimate_warps(nxt, cn, scale[3:5]), c.estimate_warps(nxt, cn, scale[3:5]))
    assert np.array_equal(c.last_stats.cpu().numpy(), runs[3][1][3:5])
    a.reset()
    assert np.array_equal(a.estimate_warps(nxt[1:], cn[1:], scale[4:5]).cpu().numpy()[0], G.IDENTITY)


def test_argument_checks_come_before_any_launch():
    from tamtr_amd import TamtrHipError, ops
    fr = torch.zeros(2, 64, 64, 3, dtype=torch.uint8, device='cuda')
    cnt = torch.ones(2, dtype=torch.int32, device='cuda')
    st = ops.gmc_state(64, 64, 'cuda')
    sc = np.ones((2, 2))
    for bad in (lambda: ops.gmc_estimate(fr.float(), cnt, sc, st), lambda: ops.gmc_estimate(fr[:, :60], cnt, sc, st),
                lambda: ops.gmc_estimate(fr.cpu(), cnt, sc, st), lambda: ops.gmc_estimate(fr, cnt.long(), sc, st),
                lambda: ops.gmc_estimate(fr, cnt, np.ones((3, 2)), st), lambda: ops.gmc_estimate(fr, cnt, sc, ops.gmc_state(128, 128, 'cuda')),
                lambda: ops.gmc_estimate(fr, cnt, sc, st, torch.empty(16, dtype=torch.uint8, device='cuda'))):
        with pytest.raises(TamtrHipError):
            bad()
    assert st['hdr'].cpu().tolist() == [0, 0, 0, 0]      # nothing ran


def test_predictor_track_keeps_ids_across_a_pan_only_with_botsort(tmp_path, monkeypatch):
    """Rectangles drawn on a textured background that the camera pans over in jumps, detections stubbed to the drawn rectangles (the
    style of test_gpu_track.py's test_predictor_track_end_to_end, with the network's detections replaced): BotSort, fed the uploaded
    frames by run_batch, keeps every id across the jumps; ByteTracker on the same input does not.  speed() has a 'gmc' entry only in
    the first case."""
    from PIL import Image
    from test_gpu_predict import CONF, IMGSZ, NC, _model, _text_feats
    from tamtr_amd import ops
    from tamtr_amd.predict import Predictor
    from tamtr_amd.track import BotSort, ByteTracker
    S, n = IMGSZ, 8
    shifts = [(0, 0), (11, -5), (0, 0), (-11, 5), (0, 0), (5, 11), (0, 0)]      # jumps of 11 px against 10 px boxes: no overlap left
    frames, truth = G.make_frames(31, S, n, [G.similarity(*t) for t in shifts])
    pos = np.array([[30., 40.], [64., 60.], [90., 35.], [50., 90.], [85., 85.]])
    src = tmp_path / 'seq'
    src.mkdir()
    boxes = []
    for t in range(n):
        pos = pos @ truth[t][:, :2].T + truth[t][:, 2]
        for k, (x, y) in enumerate(np.rint(pos).astype(int)):
            frames[t, y:y + 10, x:x + 10] = (40 * k, 255 - 40 * k, 128)
        boxes.append(np.concatenate([np.rint(pos), np.rint(pos) + 10, np.full((5, 1), 0.9), np.arange(5)[:, None] % NC], 1).astype(np.float32))
        Image.fromarray(frames[t]).save(src / f'{t:04d}.png')
    seen = [0]

    def stub(y, hw, *a, **k):      # the drawn rectangles of the batch's frames, laid out as detect_postprocess lays its outputs out
        B, nq = y.shape[0], y.shape[1]
        out = torch.zeros(B, nq, 6)
        for b in range(B):
            out[b, :5] = torch.from_numpy(boxes[seen[0] + b])
        seen[0] += B
        return out.cuda(), torch.arange(nq, dtype=torch.int32).repeat(B, 1).cuda(), torch.full((B,), 5, dtype=torch.int32).cuda()

    monkeypatch.setattr(ops, 'detect_postprocess', stub)
    names = {i: f'c{i}' for i in range(NC)}
    pred = Predictor(_model().cuda(), names, _text_feats(), imgsz=IMGSZ, conf=CONF, iou=0.7, batch=3, dtype='fp32')
    ids = {}
    for kind, trk in (('botsort', BotSort('cuda', capacity=64)), ('bytetrack', ByteTracker('cuda', capacity=64))):
        seen[0] = 0
        got = list(pred.track(str(src), tracker=trk))
        ids[kind] = [sorted(d.id.tolist()) if d.id is not None else [] for d in got]
        assert ('gmc' in pred.speed()) == (kind == 'botsort'), pred.speed()
        if kind == 'botsort':
            assert pred.speed()['gmc'] > 0 and trk.last_stats is not None and int(trk.last_stats[:, 3].sum()) > 0
    print(ids)
    assert all(f == [1, 2, 3, 4, 5] for f in ids['botsort']), ids['botsort']
    assert max(max(f) for f in ids['bytetrack'] if f) > 5, ids['bytetrack']
