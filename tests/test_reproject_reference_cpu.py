"""Motion, reprojection and jitter across frames against float64 geometry, settled without a GPU.

* frame_truth's closed loops (asserted inside pair_truth for every frame pair used here) and its camera against the view records the
  callers pass: the float64 camera and scenes.planar_view place a world point on the same window position.
* The premise of the truth: on the CPU oracle Output equals the emissive plane of the G-buffer on hit pixels, bit for bit.
* The conditions of the scenarios, from frame_truth alone (safe share, pixels with real motion, disoccluded and miss pixels).
* (a) The ideal chain -- reproject_reference's statements over the true planes -- stays inside the true hull on every safe pixel, and the
  S1 pattern separates the right jitter from the negated and the ignored one by more than a factor of two.
* (b) Twelve mutations of the ideal chain each leave the hull (or fail the S1 ratio) on at least 32 safe pixels of some scenario.
* (c) The existing float32 statement of the motion plane against the truth: this is where TAU_MV comes from.
* (d) The library's host route (the oracle's render, the float32 statements of the planes, hrpt_temporal_host / hrpt_upscale_host)
  against the ideal chain, per pixel and frame: this is where DELTA and the chain bars come from. And the host route's output lies in
  the true hull widened by the bar on every safe pixel.
* (e) Stage by stage: the statements over the host route's own planes and history against the stage's output.
* The same with the reference engine's offset convention (m_PixelOffset = jitter, offsets folded into m_MatWorldToClip), where the
  library's jitterOffsetUV term is not zero: chain, hull and stage for the upscaler, stage for the temporal pass, and the proof that a
  flipped sign or swapped views would be seen.
* One test asserts the formatted numbers that DESIGN.md section 33 prints.

The bars are module constants of reproject_cases.py, measured here and nowhere else; the GPU file uses them unchanged."""
import numpy as np
import pytest

import frame_truth as T
import reproject_cases as C
import reproject_reference as RR

F = np.float64
SPACES = [("reference-space", False), ("linear", True)]
CLAMPS = [("clamp", False), ("no-clamp", True)]
_CACHE = {}


# ---------------------------------------------------------------- the camera model and the premise
def test_camera_agrees_with_the_view_records_and_loops_close(luts):
    """The float64 camera against what scenes.planar_view hands the library (the record's matrices carried exactly): a world point lands
    on the same window position to 1e-4 px (the record is binary32) and the view depth to 1e-6 relative. pair_truth asserts its closed
    loops (X -> window -> ray -> X, X' -> w' -> ray -> X') to 1e-9 of the scene's size for every frame pair of every scenario."""
    for name in C.NAMES + ("S2w",):
        size = C.WIDE if name == "S2w" else (C.W, C.H)
        for jittered in (False, True):
            for tr in C.truths(name[:2], luts, size[0], size[1], jittered):
                t, spec = tr["truth"], tr["spec"]
                _, full = spec.constants(*size)
                hit = t["hit"]
                clip = np.concatenate([t["X"][hit], np.ones((int(hit.sum()), 1))], 1) @ np.asarray(full["m_MatWorldToClip"], F)
                win = clip[:, :2] / clip[:, 3:4] * np.asarray(full["m_ClipToWindowScale"], F) + np.asarray(full["m_ClipToWindowBias"], F)
                assert np.abs(win - t["window"][hit]).max() < 1e-4
                assert np.abs(clip[:, 3] / t["depth"][hit] - 1.0).max() < 1e-6
                assert np.array_equal(t["window"], tr["frame"].camera.samples())


@pytest.mark.parametrize("name", C.NAMES)
def test_premise_output_is_the_emissive_plane_of_the_first_hit(luts, name):
    for size, jittered in (((C.W, C.H), True), ((C.LW, C.LH), True)):
        for k, f in enumerate(C.host_inputs(name, luts, size[0], size[1], jittered)):
            hit = f["depth"][..., 0] != np.float32(1e10)
            assert 0 < hit.sum() < hit.size
            assert np.array_equal(f["colour"][hit][:, :3].view(np.uint32), f["emissive"][hit][:, :3].view(np.uint32)), (name, k)
            assert (f["colour"][..., 3] == 1).all()


# ---------------------------------------------------------------- the conditions of section 3
def test_conditions_of_the_scenarios(luts):
    assert len(C.scenario("S1", luts)[0].scene.indices) // 3 <= 300
    moving_safe, table = 0, {}
    for name in C.NAMES:
        dis_total, miss = 0, None
        for k in range(1, 4):
            t = C.truths(name, luts, C.W, C.H, False)[k]["truth"]
            safe, dis = C.safe_masks(name, luts, k, C.DELTA)
            speed = np.hypot(*t["motion"].T)
            assert (k in C.MOVING_FRAMES[name]) == (speed[t["hit"]].max() > 0.0), (name, k)
            if k in C.MOVING_FRAMES[name]:
                assert safe.sum() >= 0.30 * t["hit"].sum(), (name, k)
            moving_safe += int((safe & (speed >= 3.0)).sum())
            dis_total += int(dis.sum())
            miss = int((~t["hit"]).sum())
            table[(name, k)] = (int(safe.sum()), int(dis.sum()), miss)
        if name == "S2":
            assert dis_total >= 32 and miss >= 32
    assert moving_safe >= 200
    print("safe / disoccluded / miss per (scenario, frame):", table, "; safe pixels with |motion| >= 3 px:", moving_safe)
    assert table == C.SCENARIO_TABLE and moving_safe == C.MOVING_SAFE


# ---------------------------------------------------------------- (a) and (b): the statement against the truth
def safe(name, luts, k, consumer, size=(C.W, C.H)):
    """The safe pixels of frame k for a consumer: frame_truth's rule (reproject_cases.safe_masks) and, as the last clause of the rule
    asks, the decision margins of the unmutated ideal chain above DELTA, in both temporal spaces / both clamp modes."""
    mask, _ = C.safe_masks(name, luts, k, C.DELTA, size)
    if consumer == "temporal":
        chains = [C.ideal_temporal(name, luts, linear, None, size) for _, linear in SPACES]
    else:
        chains = [C.ideal_upscale(name, luts, no_clamp) for _, no_clamp in CLAMPS]
    for ch in chains:
        mask = mask & (ch[k]["margin"].ravel() >= C.DELTA)
    return mask


def _hull_counts(name, luts, consumer, mutation, linear=True, offsets=False, positions=None):
    """Safe pixels per frame 1..3 on which the (mutated) ideal chain leaves the true hull. positions: the number of allowed read
    positions of the upscaler's hull (None: all ten; 1: the centre's true w' alone, the hull as the issue words it)."""
    counts = []
    for k in range(1, 4):
        safe_k = safe(name, luts, k, consumer)
        if consumer == "temporal":
            ch = C.ideal_temporal(name, luts, linear, mutation)[k]
            wp = C.truths(name, luts, C.W, C.H, False)[k]["truth"]["wp"]
            v = T.hull_violation(ch["out"].reshape(-1, 4)[:, :3], ch["colour"].reshape(-1, 4)[:, :3], ch["history_in"], wp)
        else:
            ch = C.ideal_upscale(name, luts, True, mutation, offsets)[k]
            v = C.hull_violation_upscale(ch["out"].reshape(-1, 4)[:, :3], ch["cur"].reshape(-1, 3), ch["history_in"],
                                         C.upscale_read_positions(name, luts, k)[:, :positions])
        counts.append(int(((v > 0) & safe_k).sum()))
    return counts


@pytest.mark.parametrize("name", C.NAMES)
def test_ideal_chain_stays_inside_the_true_hull(luts, name):
    """On safe pixels the output lies in the hull of {G_k(p)} and the previous history at the 2 x 2 texels that enclose the TRUE w',
    per channel, widened by 1e-9 relative: the blend is monotone in both spaces and the anti-ringing clamp confines the history sample.
    The upscaler runs with HRPT_UPSCALE_NO_CLAMP (the neighbourhood clamp would hide a wrong reprojection); its history read follows the
    motion of the nearest of nine samples around the pixel, so its hull is over the texels around each of the positions those true
    motions allow (reproject_cases.upscale_read_positions). Also with the reference engine's convention (m_PixelOffset = jitter and a
    motion plane that carries the offsets' difference)."""
    for _, linear in SPACES:
        assert _hull_counts(name, luts, "temporal", None, linear) == [0, 0, 0]
    assert _hull_counts(name, luts, "upscale", None) == [0, 0, 0]
    assert _hull_counts(name, luts, "upscale", None, offsets=True) == [0, 0, 0]
    # the exclusion rule quantified: safe pixels that leave the narrower hull over the 2 x 2 texels around the centre's true w' alone
    narrow = _hull_counts(name, luts, "upscale", None, positions=1)
    print(f"{name}: the ideal upscaler leaves the hull around the centre's w' alone on {narrow} safe pixels of frames 1..3")
    assert narrow == C.NARROW_HULL_COUNTS[name]


def _s1_errors(luts, no_clamp=True):
    key = ("s1 errors", no_clamp)
    if key not in _CACHE:
        tr = C.truths("S1", luts, C.W, C.H, False)[3]
        g = tr["frame"].radiance(None, tr["truth"]).reshape(C.H, C.W, 3)
        _CACHE[key] = {m: float(np.sqrt(((C.ideal_upscale("S1", luts, no_clamp, m)[3]["out"][..., :3] - g) ** 2).mean()))
                       for m in (None, "jitter_negated", "jitter_ignored", "taps_unscaled")}
    return _CACHE[key]


def test_s1_pattern_separates_the_jitter_conventions(luts):
    """After four static frames the ideal upscaled image's RMS error against G at the display-pixel centres (whole image), and the same
    chain with the jitter negated and ignored: min(e_neg, e_zero) >= 2 e_ideal -- a condition on the pattern (reproject_cases.INDICES)."""
    for no_clamp in (True, False):
        e = _s1_errors(luts, no_clamp)
        print(f"S1 after four frames, no_clamp={no_clamp}: " + ", ".join(f"{k}: {v:.4f}" for k, v in e.items()))
        assert min(e["jitter_negated"], e["jitter_ignored"]) >= 2.0 * e[None]
    e = _s1_errors(luts)
    assert tuple(f"{e[m]:.4f}" for m in (None, "jitter_negated", "jitter_ignored", "taps_unscaled")) == C.S1_ERRORS


# mutation -> (consumer, statement's mutation, scenario, offsets convention); 'ratio': judged by the S1 RMS error
MUTATIONS = {
    "motion negated": [("temporal", "motion_negated", "S2", False), ("upscale", "motion_negated", "S2", False)],
    "motion zeroed": [("temporal", "motion_zeroed", "S2", False), ("upscale", "motion_zeroed", "S3", False)],
    "motion taken as uv": [("upscale", "motion_as_uv", "S2", False)],
    "jitterOffsetUV with the opposite sign": [("upscale", "jitter_offset_sign", "S1", True)],
    "view and prevView swapped": [("upscale", "views_swapped", "S1", True)],
    "upscaler jitter negated": "jitter_negated",
    "upscaler jitter ignored": "jitter_ignored",
    "tap offsets not scaled to display pixels": "taps_unscaled",
    "m_PrevWorld two frames old": [("temporal", "prev_world_stale", "S3", False), ("upscale", "prev_world_stale", "S3", False),
                                   ("temporal", "prev_world_stale", "S4", False), ("upscale", "prev_world_stale", "S4", False)],
    "m_PrevWorld = m_World": [("temporal", "prev_world_current", "S3", False), ("upscale", "prev_world_current", "S3", False),
                              ("temporal", "prev_world_current", "S4", False), ("upscale", "prev_world_current", "S4", False)],
    "previous vertex positions equal to the current ones": [("temporal", "prev_world_current", "S5", False), ("upscale", "prev_world_current", "S5", False)],
    "previous vertex positions not reset by the count == 0 call": [("upscale", "prev_world_stale", "S5", False)],
}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_mutations_of_the_ideal_chain_are_caught(luts, mutation):
    """Each leaves the hull on at least 32 safe pixels of some scenario. The two jitter mutations fail the S1 ratio instead, as does
    'tap offsets not scaled': it changes the taps' weights only, and a weighted mean of the taps cannot leave their hull.
    Where they are caught, as the hull sees it: 'motion taken as uv' and a reprojection that leaves the image fall back to the current
    frame in both stages, so the mutation shows where the motion is below a pixel (S2's last frame); the temporal stage's validation
    rejects it there too, the upscaler has no validation and reads 20 px away. jitterOffsetUV and the two views enter the history read of
    the upscaler only (the temporal stage uses them for the validation alone), and only where m_PixelOffset differs between frames."""
    where = MUTATIONS[mutation]
    if isinstance(where, str):
        e = _s1_errors(luts)
        print(f"{mutation}: S1 RMS error {e[where]:.4f} against {e[None]:.4f}")
        assert e[where] >= 2.0 * e[None]
        return
    caught = 0
    for consumer, m, name, offsets in where:
        counts = _hull_counts(name, luts, consumer, m, offsets=offsets)
        print(f"{mutation}: {consumer}, {name}: leaves the hull on {counts} safe pixels of frames 1..3")
        caught = max(caught, max(counts))
        assert C.MUTATION_COUNTS[(mutation, consumer, name)] == counts
    assert caught >= 32


# ---------------------------------------------------------------- (c) the motion plane against the truth
def _motion_errors(motion, tr):
    """(hit mask agrees, included, |xy| error, |z| error) of a motion plane [h, w, 4] against one entry of truths()."""
    t = tr["truth"]
    got = np.asarray(motion, F).reshape(-1, 4)
    ref = C.true_planes(tr)[0].reshape(-1, 4)
    inc = t["margin"] >= C.DELTA                 # INF on a miss that no triangle comes near
    assert set(np.unique(got[:, 3])) <= {0.0, 1.0}
    same = (got[:, 3] == 1.0) == t["hit"]
    return same, inc, np.abs(got[:, :2] - ref[:, :2]).max(1), np.abs(got[:, 2] - ref[:, 2])


def motion_check(motion, tr, what):
    """(c) for one frame: w is exactly 1 on hits and 0 on misses, the hit mask is the truth's outside the margin, xy and z to the bars."""
    same, inc, exy, ez = _motion_errors(motion, tr)
    assert (~inc).mean() <= C.MAX_EXCLUDED_SHARE, what
    assert (same | ~inc).all(), what
    ok = inc & tr["truth"]["hit"]
    worst = (float(exy[ok].max()), float(ez[ok].max()))
    assert worst[0] <= C.TAU_MV_XY and worst[1] <= C.TAU_MV_Z, (what, worst)
    return worst


def _measure_motion(luts):
    if "motion" not in _CACHE:
        worst = {}
        for name in C.NAMES + ("S2w",):
            sizes = [(C.WIDE, False)] if name == "S2w" else [((C.W, C.H), False), ((C.W, C.H), True), ((C.LW, C.LH), True)]
            wxy = wz = 0.0
            for size, jittered in sizes:
                for f, tr in zip(C.host_inputs(name[:2], luts, size[0], size[1], jittered), C.truths(name[:2], luts, size[0], size[1], jittered)):
                    same, inc, exy, ez = _motion_errors(f["motion"], tr)
                    assert (same | ~inc).all() and (~inc).mean() <= C.MAX_EXCLUDED_SHARE
                    ok = inc & tr["truth"]["hit"]
                    wxy, wz = max(wxy, float(exy[ok].max())), max(wz, float(ez[ok].max()))
            worst[name] = (wxy, wz)
        _CACHE["motion"] = worst
    return _CACHE["motion"]


def test_float32_motion_statement_against_the_truth(luts):
    """motion_reference.motion (float32, not the library) on the oracle's hits against w' - w and the true view-depth difference, on the
    planes at the pixel centres and at the render's samples, at 64 x 36, 32 x 18 and 70 x 37. TAU_MV is four times the worst deviation.
    A static frame must give exactly (0, 0, 0, 1): the truth says so (S1, S3's last frame after the caller's roll, S4's after the library's, S5's after the count == 0 call)."""
    worst = _measure_motion(luts)
    for name, (wxy, wz) in worst.items():
        print(f"{name}: float32 statement off by at most {wxy:.3e} px in xy, {wz:.3e} in z")
    assert max(w[0] for w in worst.values()) <= C.TAU_MV_XY / 3.99 and max(w[1] for w in worst.values()) <= C.TAU_MV_Z / 3.99      # the bars are 4 x the printed figures
    for name, k in (("S1", 1), ("S1", 3), ("S3", 1), ("S3", 3), ("S4", 3), ("S5", 3)):
        f, tr = C.host_inputs(name, luts, C.W, C.H, True)[k], C.truths(name, luts, C.W, C.H, True)[k]
        hit = tr["truth"]["hit"].reshape(C.H, C.W)
        assert not np.abs(tr["truth"]["motion"]).max() > 1e-12
        assert not f["motion"][hit][:, :3].view(np.uint32).any() and (f["motion"][hit][:, 3] == 1).all()


# ---------------------------------------------------------------- (d) and (e): the product's host route
def temporal_errors(frames, ideal, name, luts, size=(C.W, C.H)):
    """Per frame (included, colour error of Output, of the history, |age| error) of a product chain against the ideal chain."""
    centre, jit = C.truths(name, luts, size[0], size[1], False), C.truths(name, luts, size[0], size[1], True)
    out = []
    for k, (f, r) in enumerate(zip(frames, ideal)):
        gmax = r["colour"][..., :3].max()
        inc = (r["margin"].ravel() >= C.DELTA) & (centre[k]["truth"]["margin"] >= C.DELTA) & (jit[k]["truth"]["margin"] >= C.DELTA)
        out.append((inc, C.colour_error(f["out"], r["out"], gmax), C.colour_error(f["history"], r["history"], gmax),
                    np.abs(np.asarray(f["history"], F)[..., 3] - r["history"][..., 3]).ravel()))
    return out


def upscale_errors(frames, ideal, name, luts):
    low = C.truths(name, luts, C.LW, C.LH, True)
    out = []
    for k, (f, r) in enumerate(zip(frames, ideal)):
        gmax = low[k]["colour"][..., :3].max()
        near = low[k]["truth"]["margin"].reshape(C.LH, C.LW) < C.DELTA         # a display pixel is left out if one of its nine taps is
        j = low[k]["spec"].jitter
        bi = np.clip(np.floor((np.arange(C.W) + 0.5) * C.LW / C.W - j[0]), 0, C.LW - 1).astype(int)
        bj = np.clip(np.floor((np.arange(C.H) + 0.5) * C.LH / C.H - j[1]), 0, C.LH - 1).astype(int)
        bad = np.zeros((C.H, C.W), bool)
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                bad |= near[np.clip(bj + dj, 0, C.LH - 1)[:, None], np.clip(bi + di, 0, C.LW - 1)[None, :]]
        inc = (r["margin"].ravel() >= C.DELTA) & ~bad.ravel()
        out.append((inc, C.colour_error(f["out"], r["out"], gmax), C.colour_error(f["history"], r["history"], gmax),
                    np.abs(np.asarray(f["history"], F)[..., 3] - r["history"][..., 3]).ravel()))
    return out


def chain_check(errors, bars, what):
    """Every frame: at most 5 % left out, every included pixel within the bars (colour of the output and of the history, age / weight)."""
    worst = [0.0, 0.0, 0.0]
    left_out = 0.0
    for k, (inc, e_out, e_hist, e_w) in enumerate(errors):
        left_out = max(left_out, float((~inc).mean()))
        assert (~inc).mean() <= C.MAX_EXCLUDED_SHARE, (what, k)
        for i, e in enumerate((e_out, e_hist, e_w)):
            worst[i] = max(worst[i], float(np.where(inc, e, 0.0).max()))
        assert worst[0] <= bars[0] and worst[1] <= bars[0] and worst[2] <= bars[1], (what, k, worst)
        assert not ((np.maximum(e_out, e_hist) > 1e-2) & inc).any()
    return max(worst[0], worst[1]), worst[2], left_out


def temporal_hull_check(frames, name, luts, linear, what, size=(C.W, C.H)):
    """The product's output on safe pixels lies within the true hull (the ideal chain's colour and history) widened by TAU_TEMPORAL."""
    ideal = C.ideal_temporal(name, luts, linear, None, size)
    for k in range(1, 4):
        safe_k = safe(name, luts, k, "temporal", size)
        wp = C.truths(name, luts, size[0], size[1], False)[k]["truth"]["wp"]
        gmax = ideal[k]["colour"][..., :3].max()
        v = T.hull_violation(np.asarray(frames[k]["out"], F).reshape(-1, 4)[:, :3], ideal[k]["colour"].reshape(-1, 4)[:, :3], ideal[k]["history_in"], wp,
                             widen=C.TAU_TEMPORAL, floor=1e-3 * gmax)
        assert not ((v > 0) & safe_k).any(), (what, k)


def upscale_hull_check(frames, name, luts, what, offsets=False):
    ideal = C.ideal_upscale(name, luts, True, None, offsets)
    for k in range(1, 4):
        safe_k = safe(name, luts, k, "upscale")
        gmax = C.truths(name, luts, C.LW, C.LH, True)[k]["colour"][..., :3].max()
        v = C.hull_violation_upscale(np.asarray(frames[k]["out"], F).reshape(-1, 4)[:, :3], ideal[k]["cur"].reshape(-1, 3), ideal[k]["history_in"],
                                     C.upscale_read_positions(name, luts, k), widen=C.TAU_UPSCALE, floor=1e-3 * gmax)
        assert not ((v > 0) & safe_k).any(), (what, k)


def temporal_stage_errors(frames, linear):
    """(e): temporal64 over the chain's own read-back planes and history (binary32 carried exactly) against the stage's output."""
    out = []
    for f in frames:
        r = RR.temporal64(f["colour"], f["motion"], f["depth"], f["normal"], f["history_in"], f["view"], f["prev_view"], C.BLEND, linear)
        gmax = np.asarray(f["colour"], F)[..., :3].max()
        out.append((r["margin"].ravel() >= C.DELTA, C.colour_error(f["out"], r["out"], gmax), C.colour_error(f["history"], r["history"], gmax),
                    np.abs(np.asarray(f["history"], F)[..., 3] - r["history"][..., 3]).ravel()))
    return out


def upscale_stage_errors(frames, no_clamp):
    out = []
    for f in frames:
        r = RR.upscale64(f["colour"], f["depth"], f["motion"], f["history_in"], (C.W, C.H), f["view"], f["prev_view"], f["jitter"], kernel=C.KERNEL,
                         no_clamp=no_clamp)
        gmax = np.asarray(f["colour"], F)[..., :3].max()
        out.append((r["margin"].ravel() >= C.DELTA, C.colour_error(f["out"], r["out"], gmax), C.colour_error(f["history"], r["history"], gmax),
                    np.abs(np.asarray(f["history"], F)[..., 3] - r["history"][..., 3]).ravel()))
    return out


def _raw_worst(errors):
    """(worst included colour error, worst included age / weight error, largest share left out, largest margin-free deviation flag)."""
    colour = max(float(np.where(inc, np.maximum(a, b), 0.0).max()) for inc, a, b, _ in errors)
    weight = max(float(np.where(inc, w, 0.0).max()) for inc, _, _, w in errors)
    return colour, weight, max(float((~inc).mean()) for inc, *_ in errors)


def _measure_chains(luts):
    """{(consumer, level, scenario): (worst colour error, worst age / weight error, share left out)} over both spaces / clamp modes."""
    if "chains" not in _CACHE:
        m = {}
        for name in C.NAMES + ("S2w",):
            size = C.WIDE if name == "S2w" else (C.W, C.H)
            chain, stage = [], []
            for _, linear in SPACES:
                host = C.host_temporal(name[:2], luts, linear, size)
                chain.append(_raw_worst(temporal_errors(host, C.ideal_temporal(name[:2], luts, linear, None, size), name[:2], luts, size)))
                stage.append(_raw_worst(temporal_stage_errors(host, linear)))
            m[("temporal", "chain", name)] = tuple(max(c[i] for c in chain) for i in range(3))
            m[("temporal", "stage", name)] = tuple(max(c[i] for c in stage) for i in range(3))
            if name == "S2w":
                continue
            chain, stage = [], []
            for _, no_clamp in CLAMPS:
                host = C.host_upscale(name, luts, no_clamp)
                chain.append(_raw_worst(upscale_errors(host, C.ideal_upscale(name, luts, no_clamp), name, luts)))
                stage.append(_raw_worst(upscale_stage_errors(host, no_clamp)))
            m[("upscale", "chain", name)] = tuple(max(c[i] for c in chain) for i in range(3))
            m[("upscale", "stage", name)] = tuple(max(c[i] for c in stage) for i in range(3))
        _CACHE["chains"] = m
    return _CACHE["chains"]


@pytest.mark.parametrize("name", C.NAMES + ("S2w",))
def test_host_route_against_the_ideal_chain_and_stage_by_stage(luts, name):
    """(d) and (e) for the library's host route, both temporal spaces, the upscaler with and without HRPT_UPSCALE_NO_CLAMP. No pixel of
    any margin deviates by more than 1e-2 (asserted in chain_check on the included ones and here on all), so DELTA stays section 31's."""
    size = C.WIDE if name == "S2w" else (C.W, C.H)
    scen = name[:2]
    for label, linear in SPACES:
        host, ideal = C.host_temporal(scen, luts, linear, size), C.ideal_temporal(scen, luts, linear, None, size)
        errors = temporal_errors(host, ideal, scen, luts, size)
        assert not any((np.maximum(a, b) > 1e-2).any() for _, a, b, _ in errors)
        print(name, "temporal", label, "chain: worst colour %.3e, age %.3e, left out %.2f %%" % (lambda r: (r[0], r[1], 100 * r[2]))(
            chain_check(errors, (C.TAU_TEMPORAL, C.TAU_TEMPORAL_AGE), f"{name} temporal {label}")))
        chain_check(temporal_stage_errors(host, linear), (C.TAU_STAGE_TEMPORAL, C.TAU_STAGE_TEMPORAL_AGE), f"{name} temporal {label} stage")
        temporal_hull_check(host, scen, luts, linear, f"{name} temporal {label}", size)
    if name == "S2w":
        return
    for label, no_clamp in CLAMPS:
        host, ideal = C.host_upscale(name, luts, no_clamp), C.ideal_upscale(name, luts, no_clamp)
        errors = upscale_errors(host, ideal, name, luts)
        assert not any((np.maximum(a, b) > 1e-2).any() for _, a, b, _ in errors)
        print(name, "upscale", label, "chain: worst colour %.3e, weight %.3e, left out %.2f %%" % (lambda r: (r[0], r[1], 100 * r[2]))(
            chain_check(errors, (C.TAU_UPSCALE, C.TAU_UPSCALE_WEIGHT), f"{name} upscale {label}")))
        chain_check(upscale_stage_errors(host, no_clamp), (C.TAU_STAGE_UPSCALE, C.TAU_STAGE_UPSCALE_WEIGHT), f"{name} upscale {label} stage")
        if no_clamp:
            upscale_hull_check(host, name, luts, f"{name} upscale")


# ---------------------------------------------------------------- jitterOffsetUV in the product
OFFSET_SCENARIOS = ("S1", "S2")
OFFSET_MUTATIONS = ("jitter_offset_sign", "views_swapped")


def offset_motion_check(frames, name, luts, size, what):
    """(c) where the matrices carry the frames' offsets: the plane must be the true motion + previous offset - offset, to TAU_MV."""
    specs = C.scenario(name, luts)
    for k, (f, tr) in enumerate(zip(frames, C.truths(name, luts, size[0], size[1], True))):
        t = tr["truth"]
        ref = C.true_planes(tr, specs[max(k - 1, 0)].jitter, specs[k].jitter)[0].reshape(-1, 4)
        got = np.asarray(f["motion"], F).reshape(-1, 4)
        inc = t["hit"] & (t["margin"] >= C.DELTA)
        assert np.array_equal(got[:, 3] == 1.0, t["hit"]) or ((got[:, 3] == 1.0) == t["hit"])[t["margin"] >= C.DELTA].all()
        assert np.abs(got[:, :2] - ref[:, :2]).max(1)[inc].max() <= C.TAU_MV_XY and np.abs(got[:, 2] - ref[:, 2])[inc].max() <= C.TAU_MV_Z, (what, k)
        if k:
            assert np.abs(np.subtract(specs[k - 1].jitter, specs[k].jitter)).max() > 0.4          # the offsets do differ, by half a pixel


def offset_upscale_check(frames, name, luts, no_clamp, what):
    """A product chain run with m_PixelOffset = jitter and a motion plane that carries the offsets' difference: against the ideal chain
    of the same convention and its hull, stage by stage against upscale64 on the chain's own planes, all with DELTA and the bars of the
    plain convention -- and the stage must MISS the statement by more than its bar on at least 32 pixels of every frame with a
    predecessor once the statement takes the offset with the other sign or from the swapped views (so the agreement does depend on
    pt_upscale.h's sign and on which view it reads)."""
    assert all(tuple(np.asarray(f["view"]["m_PixelOffset"], F)) == tuple(f["jitter"]) for f in frames)
    chain_check(upscale_errors(frames, C.ideal_upscale(name, luts, no_clamp, None, True), name, luts), (C.TAU_UPSCALE, C.TAU_UPSCALE_WEIGHT), what)
    chain_check(upscale_stage_errors(frames, no_clamp), (C.TAU_STAGE_UPSCALE, C.TAU_STAGE_UPSCALE_WEIGHT), what + ", stage")
    if no_clamp:
        upscale_hull_check(frames, name, luts, what, offsets=True)
    for m in OFFSET_MUTATIONS:
        for k, f in enumerate(frames[1:], start=1):
            r = RR.upscale64(f["colour"], f["depth"], f["motion"], f["history_in"], (C.W, C.H), f["view"], f["prev_view"], f["jitter"], kernel=C.KERNEL,
                             no_clamp=no_clamp, mutation=m)
            e = C.colour_error(f["out"], r["out"], np.asarray(f["colour"], F)[..., :3].max())
            assert (e > C.TAU_STAGE_UPSCALE).sum() >= 32, (what, m, k)


def offset_temporal_check(frames, linear, what):
    """The same for the temporal stage, stage by stage (its jitterOffsetUV enters the validation alone): temporal64 over the chain's
    own planes within the stage bars, and beyond them on at least 32 pixels per frame with the sign flipped or the views swapped."""
    assert all(np.abs(np.asarray(f["view"]["m_PixelOffset"], F)).max() > 0.2 for f in frames)
    chain_check(temporal_stage_errors(frames, linear), (C.TAU_STAGE_TEMPORAL, C.TAU_STAGE_TEMPORAL_AGE), what + ", stage")
    for m in OFFSET_MUTATIONS:
        for k, f in enumerate(frames[1:], start=1):
            r = RR.temporal64(f["colour"], f["motion"], f["depth"], f["normal"], f["history_in"], f["view"], f["prev_view"], C.BLEND, linear, m)
            e = C.colour_error(f["out"], r["out"], np.asarray(f["colour"], F)[..., :3].max())
            assert (e > C.TAU_STAGE_TEMPORAL).sum() >= 32, (what, m, k)


@pytest.mark.parametrize("name", OFFSET_SCENARIOS)
def test_host_route_with_the_reference_engines_offset_convention(luts, name):
    """Every other product run here passes views whose m_PixelOffset is 0, so the library's jitterOffsetUV term is 0 there. Here the
    frame's jitter is folded into m_MatWorldToClip of both views and stated in m_PixelOffset (Spec.constants(offsets=True)): the
    motion plane then carries (previous offset - offset), half a pixel between any two frames, and hrpt_temporal_host / hrpt_upscale_host
    must take it out again -- with the sign and from the views the shader text says."""
    for size in ((C.W, C.H), (C.LW, C.LH)):
        offset_motion_check(C.host_inputs(name, luts, size[0], size[1], True, True), name, luts, size, f"{name} {size}")
    for label, no_clamp in CLAMPS:
        offset_upscale_check(C.host_upscale(name, luts, no_clamp, True), name, luts, no_clamp, f"{name}, offsets, upscale {label}")
    for label, linear in SPACES:
        offset_temporal_check(C.host_temporal(name, luts, linear, (C.W, C.H), True, True), linear, f"{name}, offsets, temporal {label}")


def test_which_jitter_the_temporal_stage_wants_for_its_planes(luts):
    """With the planes at the pixel centres (m_Jitter = 0, as test_temporal_gpu.py renders them) the history is read at exactly the true
    w' of the pixel's centre. With the planes at the render's samples the read position is w'(sample) - jitter: the same to first order,
    off by the change of the motion across the sub-pixel offset. Both stay inside the true hull on every safe pixel of these scenarios;
    the largest distance between the two read positions on a safe pixel is recorded."""
    worst = 0.0
    for name in C.NAMES:
        centre = C.ideal_temporal(name, luts, True)
        jittered = C.ideal_temporal(name, luts, True, jittered_planes=True)
        for k in range(1, 4):
            safe_k = safe(name, luts, k, "temporal")
            t = C.truths(name, luts, C.W, C.H, False)[k]["truth"]
            assert np.abs(centre[k]["reproj"].reshape(-1, 2)[safe_k] * (C.W, C.H) - t["wp"][safe_k]).max() < 1e-9
            worst = max(worst, float(np.abs(jittered[k]["reproj"].reshape(-1, 2)[safe_k] * (C.W, C.H) - t["wp"][safe_k]).max()))
            v = T.hull_violation(jittered[k]["out"].reshape(-1, 4)[:, :3], jittered[k]["colour"].reshape(-1, 4)[:, :3], jittered[k]["history_in"], t["wp"])
            assert not ((v > 0) & safe_k).any()
    print(f"planes at the render's samples: the history read is off the true w' of the centre by at most {worst:.3f} px")
    assert f"{worst:.3f}" == C.JITTERED_PLANES_BIAS


# ---------------------------------------------------------------- the numbers of DESIGN.md section 33
def test_delta_and_tau_are_what_the_host_route_measures(luts):
    """DELTA, TAU_MV and the chain and stage bars follow section 31's recipe from the figures measured above; the formatted numbers are
    those DESIGN.md section 33 prints."""
    import path_reference as R
    assert C.DELTA == R.DELTA == 2.0 ** -19
    motion = _measure_motion(luts)
    chains = _measure_chains(luts)
    got_motion = {k: (f"{v[0]:.3e}", f"{v[1]:.3e}") for k, v in motion.items()}
    got_chains = {k: (f"{v[0]:.3e}", f"{v[1]:.3e}", f"{100 * v[2]:.2f}") for k, v in chains.items()}
    print(got_motion)
    print(got_chains)
    assert got_motion == C.MOTION_TABLE
    assert got_chains == C.CHAIN_TABLE
    worst = lambda consumer, level, i: max(float(v[i]) for k, v in C.CHAIN_TABLE.items() if k[0] == consumer and k[1] == level)      # noqa: E731
    assert C.TAU_MV_XY == 4.0 * max(float(v[0]) for v in C.MOTION_TABLE.values()) and C.TAU_MV_Z == 4.0 * max(float(v[1]) for v in C.MOTION_TABLE.values())
    assert C.TAU_TEMPORAL == 4.0 * worst("temporal", "chain", 0) and C.TAU_TEMPORAL_AGE == 4.0 * worst("temporal", "chain", 1)
    assert C.TAU_UPSCALE == 4.0 * worst("upscale", "chain", 0) and C.TAU_UPSCALE_WEIGHT == 4.0 * worst("upscale", "chain", 1)
    assert C.TAU_STAGE_TEMPORAL == 4.0 * worst("temporal", "stage", 0) and C.TAU_STAGE_TEMPORAL_AGE == 4.0 * worst("temporal", "stage", 1)
    assert C.TAU_STAGE_UPSCALE == 4.0 * worst("upscale", "stage", 0) and C.TAU_STAGE_UPSCALE_WEIGHT == 4.0 * worst("upscale", "stage", 1)
