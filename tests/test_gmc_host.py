"""CPU: the numpy statement of the camera-motion estimate (tests/gmc_np.py, the twin of csrc/gmc.hip) against synthetic ground truth.

The condition on a warp is geometric and comes from the use, not from the code: it must map the four frame corners to within half a
pixel of where the true warp maps them - VisDrone's boxes are a few pixels wide, and a compensation coarser than that is none."""
import functools

import numpy as np
import pytest

import gmc_np as G

CASES = [(256, 0, 1), (256, 2, 2), (128, 0, 3), (128, 2, 4)]      # S, movers, seed: 4 and 3 pyramid levels


@functools.lru_cache(maxsize=None)
def case(S, movers, seed):
    """Three frames under random similarities (translation up to 12 px, rotation up to 2 degrees, scale 0.98 .. 1.02), run through the
    twin in fp64 and in fp32.  Shared by the tests below and by tests/test_gpu_gmc.py; nothing in it is changed afterwards."""
    motions = G.random_motions(seed + 10 * S, 2, S=S)
    frames, truth = G.make_frames(seed, S, 3, motions, movers)
    w64, s64 = G.GmcNp(np.float64).estimate(frames, [1, 1, 1])
    w32, s32 = G.GmcNp(np.float32).estimate(frames, [1, 1, 1])
    return frames, truth, (w64, s64), (w32, s32)


def test_levels_and_integer_stages_by_hand():
    assert [G.n_levels(s, s) for s in (64, 128, 256, 640)] == [2, 3, 4, 4] and G.n_levels(72, 136) == 2
    rgb = np.zeros((8, 8, 3), np.uint8)
    rgb[..., 0], rgb[..., 1], rgb[..., 2] = 255, 10, 3
    assert G.grey(rgb)[0, 0] == (77 * 255 + 150 * 10 + 29 * 3 + 128) >> 8
    flat = np.full((16, 16), 200, np.uint8)
    assert np.array_equal(G.pyr_down(flat), np.full((8, 8), 200, np.uint8))      # the weights sum to 256: a flat image stays flat
    ramp = np.tile(np.arange(0, 64, 4, dtype=np.uint8), (16, 1))
    assert np.array_equal(G.pyr_down(ramp)[:, 1:-1], ramp[::2, ::2][:, 1:-1])    # and a ramp keeps its values away from the border
    assert G.corner_response(flat).max() == 0 and (G.keypoints(G.corner_response(np.tile(flat, (4, 4)))) == -1).all()


def test_hypothesis_pairs_are_distinct_and_in_range():
    for n in (5, 64, 1024):
        ij = np.array([G.hypothesis(k, n) for k in range(G.HYP)])
        assert (ij >= 0).all() and (ij < n).all() and (ij[:, 0] != ij[:, 1]).all() and len({tuple(p) for p in ij.tolist()}) > min(n, 100)


@pytest.mark.parametrize('S,movers,seed', CASES)
def test_twin_meets_the_half_pixel_condition(S, movers, seed):
    _, truth, (w64, s64), _ = case(S, movers, seed)
    assert np.array_equal(w64[0], G.IDENTITY) and not s64[0].any()      # the first frame of a sequence
    for t in (1, 2):
        err = G.corner_error(w64[t], truth[t], S, S)
        kp, tracked, inl, used = s64[t]
        print(f'S {S} movers {movers} frame {t}: corner error {err:.3f} px, keypoints {kp}, tracked {tracked}, inliers {inl}')
        assert used == 1 and err <= 0.5
        assert tracked > 200 and (inl < tracked if movers else inl > tracked // 2)      # with movers the fit did reject something


@pytest.mark.parametrize('S,movers,seed', CASES)
def test_fp32_and_fp64_agree_on_every_status(S, movers, seed):
    """The precondition of the GPU test's 1 % cap: on these inputs no point's lost / kept decision hangs on the precision."""
    frames = case(S, movers, seed)[0]
    pyr = [G.pyramid(G.grey(f)) for f in frames[:2]]
    kp = G.keypoints(G.corner_response(pyr[0][0]))
    p64, s64 = G.lk(pyr[0], pyr[1], kp, np.float64)
    p32, s32 = G.lk(pyr[0], pyr[1], kp, np.float32)
    assert p32.dtype == np.float32 and np.array_equal(s64, s32)
    both = s64 == 2
    assert np.abs(p32[both] - p64[both]).max() < 0.05      # fp32 noise, far below the half pixel


def test_pairing_across_empty_frames_and_batches():
    S = 64
    motions = [G.similarity(3, -2), G.similarity(-2, 3), G.similarity(2, 2), G.similarity(-3, 1), G.similarity(1, -3)]
    frames, truth = G.make_frames(7, S, 6, motions)
    counts = [2, 0, 5, 0, 1, 3]
    one = G.GmcNp()
    w, s = one.estimate(frames, counts)
    assert one.pairs == [None, None, 0, None, 2, 4]
    for b in (0, 1, 3):
        assert np.array_equal(w[b], G.IDENTITY) and not s[b].any()      # first frame; empty frames get no warp
    span = lambda a, b: (np.vstack([truth[b], [0, 0, 1]]) @ np.vstack([truth[a], [0, 0, 1]]))[:2]      # noqa: E731  two frames' motion
    assert G.corner_error(w[2], span(1, 2), S, S) <= 0.5 and G.corner_error(w[4], span(3, 4), S, S) <= 0.5
    assert G.corner_error(w[5], truth[5], S, S) <= 0.5
    # the same frames in batches of 1, 2 and 3 with the state carried over: the same warps, bit for bit
    parts = G.GmcNp()
    got = [parts.estimate(frames[a:b], counts[a:b]) for a, b in ((0, 1), (1, 3), (3, 6))]
    assert np.array_equal(np.concatenate([g[0] for g in got]), w) and np.array_equal(np.concatenate([g[1] for g in got]), s)
    assert parts.pairs == [None, 'state', 1]      # the last batch: an empty frame, the state, the frame before
    # a batch of empty frames leaves the state alone; reset() forgets it
    prev = parts.prev
    parts.estimate(frames[:2], [0, 0])
    assert parts.prev is prev
    parts.reset()
    assert np.array_equal(parts.estimate(frames[5:], [1])[0][0], G.IDENTITY)


def test_fit_rejects_outliers_and_small_sets_give_identity():
    rng = np.random.default_rng(5)
    M = G.similarity(4.5, -7.25, 1.5, 1.01, centre=(100, 100))
    for n in (5, 64, 1024):
        src = rng.uniform(0, 200, (n, 2))
        dst = src @ M[:, :2].T + M[:, 2] + rng.normal(0, 0.05, (n, 2))
        bad = rng.random(n) < 0.3
        bad[:4] = False
        dst[bad] += rng.uniform(8, 30, (int(bad.sum()), 2))
        warp, k, mask, used = G.fit(src, dst)
        assert used and 0 <= k < G.HYP and not mask[bad].any() and mask.sum() >= 0.9 * (~bad).sum()
        assert G.corner_error(warp, M, 200, 200) < (0.5 if n == 5 else 0.1)
    warp, k, mask, used = G.fit(src[:4], dst[:4])
    assert np.array_equal(warp, G.IDENTITY) and k == -1 and not used
