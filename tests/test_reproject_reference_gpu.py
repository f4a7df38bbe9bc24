"""The device against float64 geometry across frames: (c) the motion plane against frame_truth, (d) the real chain
hrpt_render -> hrpt_render_motion_vectors -> hrpt_temporal_accumulate / hrpt_upscale against the ideal chain, each side feeding its own
history forward, and (e) every stage against reproject_reference's statement over the device's own read-back planes and history. DELTA,
the bars and the 5 % cap are those tests/test_reproject_reference_cpu.py settled on the CPU; nothing is adjusted here.

Covered: scenarios S1 - S5 on the wavefront and the megakernel paths for the render and the planes, S3 (hrpt_update_instances, the
caller's m_PrevWorld roll), S4 (hrpt_animate on the device) and S5 (hrpt_update_vertices) also over HRPT_ACCEL_TWO_LEVEL, S5 with the
host builder and with a GPU builder plus HRPT_VERTICES_REFIT, both temporal spaces, the upscaler with and without
HRPT_UPSCALE_NO_CLAMP through the gather and the staged kernel, S2 at 70 x 37 (ragged 32 x 8 tiles), S1 and S2 with the reference engine's offset
convention (m_PixelOffset = jitter: the kernels' jitterOffsetUV term is not zero), and the device's worst figures against the host
route's table."""
import numpy as np
import pytest

from hobbyrenderer_amd import structs as S
import reproject_cases as C
import test_reproject_reference_cpu as CPU

pytestmark = pytest.mark.gpu
KERNELS = [("wavefront", S.FRAME_WAVEFRONT), ("megakernel", S.FRAME_MEGAKERNEL)]


def _context(scene, structure=None, builder=None):
    from hobbyrenderer_amd.native import PathTracerContext
    ctx = PathTracerContext(0)
    try:
        if builder is not None:
            ctx.set_bvh_builder(builder)
        if structure is not None:
            ctx.set_acceleration_structure(structure)
        ctx.upload_scene(scene)
        if structure is not None:
            assert ctx.build_info().structure == structure
    except Exception:
        ctx.close()
        raise
    return ctx


def _advance(ctx, spec, records, vertex_flags=0, animation=None):
    """What the caller tells the library at the start of a frame: hrpt_animate at the frame's time (and, after it, the one record the
    caller moves itself), or instance records that changed (hrpt_update_instances with the caller's m_PrevWorld); vertex ranges that
    deformed (the second and later ones with HRPT_VERTICES_SAME_FRAME), or the count == 0 call."""
    if spec.animate is not None:
        animation.set_times([spec.animate])
        ctx.animate(animation)
        if spec.update_one is not None:
            ctx.update_instances(spec.scene.instances[spec.update_one:spec.update_one + 1], spec.update_one)
        records = spec.scene.instances
    elif spec.scene.instances.tobytes() != records.tobytes():
        records = spec.scene.instances
        ctx.update_instances(records, 0)
    for n, (first, count) in enumerate(spec.vertex_ranges or ()):
        ctx.update_vertices(spec.scene.vertices[first:first + count], first, vertex_flags | (S.VERTICES_SAME_FRAME if n else 0))
        if vertex_flags & S.VERTICES_REFIT:
            assert ctx.build_info().usedBuilder & S.BVH_BUILDER_REFITTED, hex(ctx.build_info().usedBuilder)
    if spec.end_vertex_frame:
        ctx.end_vertex_frame()
    return records


def _animation(specs):
    from hobbyrenderer_amd import native
    return native.Animation(**C.animation_tables()) if any(s.animate is not None for s in specs) else None


def _frames(name, luts, size, flags, structure, stage, builder=None, vertex_flags=0, offsets=False):
    """The documented frame order on the device. stage.planes(spec) -> (the planes' m_Jitter, the plane mask); stage.run(...) runs the
    consumer and reads its output and history back. Returns the per-frame dicts of reproject_cases' host chains (colour, motion, depth,
    normal, view, prev_view, out, history, history_in, jitter)."""
    specs = C.scenario(name, luts)
    w, h = size
    ctx = _context(specs[0].scene, structure, builder)
    animation = _animation(specs)
    out = []
    try:
        ctx.resize(w, h)
        prev_full, history, records = None, None, specs[0].scene.instances
        for k, spec in enumerate(specs):
            records = _advance(ctx, spec, records, vertex_flags, animation)
            cb, full = spec.constants(w, h, offsets=offsets)
            prev = full if prev_full is None else prev_full
            jitter, mask = stage.planes(spec)
            cbm, _ = spec.constants(w, h, jitter, offsets=offsets)
            ctx.clear_accumulation()
            ctx.render(cb, accum_count=1, flags=flags)
            ctx.render_motion_vectors(cbm, prev, planes=mask, flags=flags)
            f = dict(colour=ctx.read_output(), motion=ctx.read_motion_vectors(), depth=ctx.read_gbuffer(S.GB_DEPTH),
                     normal=ctx.read_gbuffer(S.GB_NORMAL) if mask & (1 << S.GB_NORMAL) else None,
                     view=full, prev_view=prev, history_in=history, jitter=spec.jitter)
            f["out"], f["history"] = stage.run(ctx, spec, full, prev)
            out.append(f)
            prev_full, history = full, f["history"]
    finally:
        ctx.close()
        if animation is not None:
            animation.close()
    return out


class _Temporal:
    def __init__(self, linear, jittered_planes=False):
        self.params = S.TemporalParams(C.BLEND, S.TEMPORAL_LINEAR if linear else 0)
        self.jittered_planes = jittered_planes

    def planes(self, spec):
        return (spec.jitter if self.jittered_planes else (0.0, 0.0)), (1 << S.GB_DEPTH) | (1 << S.GB_NORMAL)

    def run(self, ctx, spec, full, prev):
        ctx.temporal_accumulate(full, prev, self.params)
        return ctx.read_output(), ctx.read_temporal_history()


class _Upscale:
    def __init__(self, no_clamp):
        self.flags = S.UPSCALE_NO_CLAMP if no_clamp else 0

    def planes(self, spec):
        return spec.jitter, 1 << S.GB_DEPTH

    def run(self, ctx, spec, full, prev):
        ctx.upscale(C.W, C.H, full, prev, S.UpscaleParams(jitter=spec.jitter, kernel=C.KERNEL, flags=self.flags))
        return ctx.read_upscaled(), ctx.read_upscale_history()


def _check_temporal(name, luts, linear, flags, structure=None, size=(C.W, C.H), what="", builder=None, vertex_flags=0):
    frames = _frames(name, luts, size, flags, structure, _Temporal(linear), builder, vertex_flags)
    ideal = C.ideal_temporal(name, luts, linear, None, size)
    worst = CPU.chain_check(CPU.temporal_errors(frames, ideal, name, luts, size), (C.TAU_TEMPORAL, C.TAU_TEMPORAL_AGE), what)
    stage = CPU.chain_check(CPU.temporal_stage_errors(frames, linear), (C.TAU_STAGE_TEMPORAL, C.TAU_STAGE_TEMPORAL_AGE), what + ", stage")
    CPU.temporal_hull_check(frames, name, luts, linear, what, size)
    for k, (f, tr) in enumerate(zip(frames, C.truths(name, luts, size[0], size[1], False))):                  # (c) on the planes at the pixel centres
        CPU.motion_check(f["motion"], tr, f"{what}, frame {k}")
    print(f"{what}: chain worst colour {worst[0]:.3e}, age {worst[1]:.3e}, {100 * worst[2]:.2f} % left out; stage worst colour {stage[0]:.3e}, age {stage[1]:.3e}")
    return worst, stage


def _check_upscale(name, luts, no_clamp, flags, structure=None, what="", builder=None, vertex_flags=0):
    frames = _frames(name, luts, (C.LW, C.LH), flags, structure, _Upscale(no_clamp), builder, vertex_flags)
    ideal = C.ideal_upscale(name, luts, no_clamp)
    worst = CPU.chain_check(CPU.upscale_errors(frames, ideal, name, luts), (C.TAU_UPSCALE, C.TAU_UPSCALE_WEIGHT), what)
    stage = CPU.chain_check(CPU.upscale_stage_errors(frames, no_clamp), (C.TAU_STAGE_UPSCALE, C.TAU_STAGE_UPSCALE_WEIGHT), what + ", stage")
    if no_clamp:
        CPU.upscale_hull_check(frames, name, luts, what)
    for k, (f, tr) in enumerate(zip(frames, C.truths(name, luts, C.LW, C.LH, True))):                        # (c) on the planes at the render's samples
        CPU.motion_check(f["motion"], tr, f"{what}, frame {k}")
    print(f"{what}: chain worst colour {worst[0]:.3e}, weight {worst[1]:.3e}, {100 * worst[2]:.2f} % left out; stage worst colour {stage[0]:.3e}, weight {stage[1]:.3e}")
    return worst, stage


@pytest.mark.parametrize("label,flags", KERNELS)
@pytest.mark.parametrize("space,linear", CPU.SPACES)
@pytest.mark.parametrize("name", C.NAMES)
def test_temporal_chain_against_the_ideal_chain(luts, name, space, linear, label, flags):
    _check_temporal(name, luts, linear, flags, what=f"{name}, temporal, {space}, {label}")


@pytest.mark.parametrize("label,flags", KERNELS)
@pytest.mark.parametrize("clamp,no_clamp", CPU.CLAMPS)
@pytest.mark.parametrize("name", C.NAMES)
def test_upscale_chain_against_the_ideal_chain(luts, name, clamp, no_clamp, label, flags):
    _check_upscale(name, luts, no_clamp, flags, what=f"{name}, upscale, {clamp}, {label}")


@pytest.mark.parametrize("name", C.NAMES + ("S2w",))
def test_device_figures_are_the_host_routes(luts, name):
    """The worst included errors of the device's chains and stages (wavefront path, both temporal spaces, both clamp modes), formatted as
    DESIGN.md section 33 prints them, equal the host route's in reproject_cases.CHAIN_TABLE: the device reproduces the table."""
    size, scen = (C.WIDE, "S2") if name == "S2w" else ((C.W, C.H), name)
    got = [_check_temporal(scen, luts, linear, S.FRAME_WAVEFRONT, size=size, what=f"{name}, temporal, {space}") for space, linear in CPU.SPACES]
    fmt = lambda rows, i: tuple(f"{max(r[i][j] for r in rows):.3e}" for j in (0, 1))      # noqa: E731
    assert fmt(got, 0) == C.CHAIN_TABLE[("temporal", "chain", name)][:2] and fmt(got, 1) == C.CHAIN_TABLE[("temporal", "stage", name)][:2]
    if name != "S2w":
        got = [_check_upscale(name, luts, no_clamp, S.FRAME_WAVEFRONT, what=f"{name}, upscale, {clamp}") for clamp, no_clamp in CPU.CLAMPS]
        assert fmt(got, 0) == C.CHAIN_TABLE[("upscale", "chain", name)][:2] and fmt(got, 1) == C.CHAIN_TABLE[("upscale", "stage", name)][:2]


@pytest.mark.parametrize("name", CPU.OFFSET_SCENARIOS)
def test_reference_engines_offset_convention_on_the_device(luts, name):
    """The real chain with the frame's jitter folded into m_MatWorldToClip of both views and stated in m_PixelOffset, so that
    hrpt_render_motion_vectors' plane carries (previous offset - offset) and jitterOffsetUV in the two kernels is not zero: the checks of
    test_host_route_with_the_reference_engines_offset_convention, the upscaler through both kernel paths of render and planes."""
    for label, flags in KERNELS:
        frames = _frames(name, luts, (C.LW, C.LH), flags, None, _Upscale(True), offsets=True)
        CPU.offset_motion_check(frames, name, luts, (C.LW, C.LH), f"{name}, offsets, {label}")
        CPU.offset_upscale_check(frames, name, luts, True, f"{name}, offsets, upscale no-clamp, {label}")
    frames = _frames(name, luts, (C.LW, C.LH), S.FRAME_WAVEFRONT, None, _Upscale(False), offsets=True)
    CPU.offset_upscale_check(frames, name, luts, False, f"{name}, offsets, upscale clamp")
    for space, linear in CPU.SPACES:
        frames = _frames(name, luts, (C.W, C.H), S.FRAME_WAVEFRONT, None, _Temporal(linear, jittered_planes=True), offsets=True)
        CPU.offset_motion_check(frames, name, luts, (C.W, C.H), f"{name}, offsets, temporal {space}")
        CPU.offset_temporal_check(frames, linear, f"{name}, offsets, temporal {space}")


@pytest.mark.parametrize("name", C.NAMES)
def test_staged_upscale_kernel_against_the_ideal_chain(luts, name, monkeypatch):
    monkeypatch.setenv("HRPT_UPSCALE_STAGED", "1")              # a context knob, read at hrpt_create
    for clamp, no_clamp in CPU.CLAMPS:
        _check_upscale(name, luts, no_clamp, S.FRAME_WAVEFRONT, what=f"{name}, upscale, {clamp}, staged kernel")


@pytest.mark.parametrize("label,flags", KERNELS)
@pytest.mark.parametrize("name", ["S3", "S4"])
def test_instance_protocol_over_the_two_level_structure(luts, name, label, flags):
    """S6: S3 and S4 over HRPT_ACCEL_TWO_LEVEL, where hrpt_update_instances and hrpt_animate rebuild the instance tree; the caller's
    m_PrevWorld roll of section 16 and the library's own of section 23."""
    _check_temporal(name, luts, True, flags, S.ACCEL_TWO_LEVEL, what=f"{name}, two-level, temporal, linear, {label}")
    _check_upscale(name, luts, True, flags, S.ACCEL_TWO_LEVEL, what=f"{name}, two-level, upscale, no-clamp, {label}")


@pytest.mark.parametrize("builder", [S.BVH_BUILDER_GPU_LBVH, S.BVH_BUILDER_GPU_PLOC], ids=["lbvh", "ploc"])
def test_vertex_protocol_with_a_gpu_builder_and_refit(luts, builder):
    """S5 with a GPU builder holding the geometry and HRPT_VERTICES_REFIT on both ranges: the previous-position protocol of section 21
    (two ranges in one frame, then the count == 0 call) where the tree is refitted, not rebuilt."""
    _check_temporal("S5", luts, True, S.FRAME_WAVEFRONT, builder=builder, vertex_flags=S.VERTICES_REFIT, what="S5, GPU builder + refit, temporal, linear")
    _check_upscale("S5", luts, True, S.FRAME_WAVEFRONT, builder=builder, vertex_flags=S.VERTICES_REFIT, what="S5, GPU builder + refit, upscale, no-clamp")


def test_vertex_protocol_over_the_two_level_structure(luts):
    _check_temporal("S5", luts, True, S.FRAME_WAVEFRONT, S.ACCEL_TWO_LEVEL, what="S5, two-level, temporal, linear")
    _check_upscale("S5", luts, True, S.FRAME_MEGAKERNEL, S.ACCEL_TWO_LEVEL, what="S5, two-level, upscale, no-clamp, megakernel")


@pytest.mark.parametrize("space,linear", CPU.SPACES)
def test_ragged_tiles_at_70_by_37(luts, space, linear):
    _check_temporal("S2", luts, linear, S.FRAME_WAVEFRONT, size=C.WIDE, what=f"S2 at 70 x 37, temporal, {space}")


def test_motion_plane_with_the_renders_jitter_at_full_size(luts):
    """(c) at 64 x 36 with m_Jitter = the render's Halton point, on both paths: the sign of m_Jitter in raygen against p + 0.5 + jitter."""
    for name in C.NAMES:
        specs = C.scenario(name, luts)
        ctx = _context(specs[0].scene)
        animation = _animation(specs)
        try:
            ctx.resize(C.W, C.H)
            prev_full, records = None, specs[0].scene.instances
            for k, (spec, tr) in enumerate(zip(specs, C.truths(name, luts, C.W, C.H, True))):
                records = _advance(ctx, spec, records, animation=animation)
                cbm, full = spec.constants(C.W, C.H, spec.jitter)
                planes = []
                for label, flags in KERNELS:
                    ctx.render_motion_vectors(cbm, full if prev_full is None else prev_full, flags=flags)
                    planes.append(ctx.read_motion_vectors())
                    CPU.motion_check(planes[-1], tr, f"{name}, frame {k}, {label}")
                assert np.array_equal(planes[0].view(np.uint32), planes[1].view(np.uint32))
                prev_full = full
        finally:
            ctx.close()
            if animation is not None:
                animation.close()
