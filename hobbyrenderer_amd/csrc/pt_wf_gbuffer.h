// pt_wf_gbuffer.h -- the first-hit images: wf_gbuffer (hrpt_render_gbuffer: albedo, normal, depth and id planes from the hit records of a
// one-sample-per-pixel batch) and wf_gbuffer_motion (hrpt_render_motion_vectors: the same with the screen-space motion of the hit).
// A piece of pt_wavefront.hip, included there after pt_gbuffer.h, pt_motion.h and pt_wf_common.h: no stand-alone header.
// ------------------------------------------------------------------ first-hit G-buffer (hrpt_render_gbuffer)
// Runs after wf_raygen + wf_extend(0) of a one-sample-per-pixel batch: persistent waves over the segments of path queue 0, like wf_shade. A lane
// takes one path, reads its ray, sample index and hit record (+ instance on two-level scenes), gathers the triangle / instance / material records
// from global memory, evaluates gbuffer_texels (pt_gbuffer.h: full_hit_attributes + pbr_attributes, the code wf_shade runs) and stores one float4
// per requested plane at the sample's pixel. wf_raygen enumerates samples in 8 x 8 pixel tiles and compacts only the padding away, so eight
// consecutive lanes hold eight consecutive pixels of a row: each plane store of a wave covers whole 128-byte row pieces. planeMask is a kernel
// argument: the stores are the only code it guards. No shading-class sort and no LDS tables (wf_shade's answers to its long divergent branches and
// its thirteen gathers per path): this kernel's divergent part is pbr_attributes alone, see DESIGN.md section 15.
__global__ __launch_bounds__(kBlock) void wf_gbuffer(WfArgs a, HrptPathTracerConstants cb, GBufferPlanes g, uint32_t planeMask)
{
    const uint32_t wavesPerBlock = kBlock / 64, lane = lane_id();
    const uint32_t gw = uniform(blockIdx.x * wavesPerBlock + (threadIdx.x >> 6)), totalWaves = gridDim.x * wavesPerBlock;
    const SceneView& s = a.scene;
    for (uint32_t seg = gw; seg < a.numSegments; seg += totalWaves) {
        const uint32_t cnt = uniform(a.b.pathCnt[0][seg]), segBase = seg * a.segSize;
        for (uint32_t base = 0; base < cnt; base += 64) {
            if (base + lane >= cnt) continue;
            const uint32_t slot = segBase + base + lane;
            const float4 o = a.b.rayO[0][slot], d = a.b.rayD[0][slot], ha = a.b.hit[slot];
            const uint32_t smp = reinterpret_cast<const uint32_t*>(a.b.thr[0] + slot)[3];       // one accumulation index: sample == padded pixel
            const uint32_t tile = smp >> 6, within = smp & 63u;
            // tile_position with selects instead of two arms (as two arms the compiler parked the quotient / remainder pair in scratch here)
            const bool columnMajor = a.rect.stripeCount > 1u;
            const uint32_t den = columnMajor ? a.tilesY : a.tilesX, quo = tile / den, rem = tile - quo * den;
            const uint32_t tcol = columnMajor ? quo : rem, trow = columnMajor ? rem : quo;
            const uint32_t px = a.rect.column_x(tcol) + (within & 7u), py = a.rect.y0 + trow * 8u + (within >> 3);
            uint32_t tri = __float_as_uint(ha.w);
            float4 texel[kGbPlanes];
            if (tri != 0xFFFFFFFFu) {
                tri &= 0x1FFFFFFFu;                                  // bits 29-31: shading class (wf_extend)
                Ray ray; ray.o = mk3(o.x, o.y, o.z); ray.d = mk3(d.x, d.y, d.z); ray.tmin = o.w; ray.tmax = 1e10f;
                Hit h; h.valid = true; h.t = ha.x; h.u = ha.y; h.v = ha.z; h.tri = tri; h.prim = 0; h.inst = s.instances ? a.b.hitInst[slot] : 0u; h.opaque = 1;
                gbuffer_texels(s, cb, ray, h, texel);
            } else gbuffer_miss(texel);
            gbuffer_store(g, planeMask, (size_t)py * a.imageWidth + px, texel);
        }
    }
}

// ------------------------------------------------------------------ first-hit motion vectors (hrpt_render_motion_vectors)
// wf_gbuffer's loop with one more plane: the motion texel of pt_motion.h (16 bytes per pixel), and the G-buffer texels only when the call names
// G-buffer planes too (PLANES = planeMask != 0: one traversal serves both; the motion-only instantiation carries none of gbuffer_texels'
// registers). Held to four waves per SIMD (at most 128 VGPRs) like the shade kernels. The motion gather -- instance record, three indices, three positions, a
// three-deep dependent chain -- is issued before gbuffer_texels so that it is in flight while pbr_attributes waits for its texels; lanes that
// missed skip it and store zeros. The pixel lookup is wf_gbuffer's, restated here: that kernel stays the one hrpt_render_gbuffer has always run.
template <bool PLANES>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4))) void wf_gbuffer_motion(WfArgs a, HrptPathTracerConstants cb, GBufferPlanes g, uint32_t planeMask, MotionArgs m)
{
    const uint32_t wavesPerBlock = kBlock / 64, lane = lane_id();
    const uint32_t gw = uniform(blockIdx.x * wavesPerBlock + (threadIdx.x >> 6)), totalWaves = gridDim.x * wavesPerBlock;
    const SceneView& s = a.scene;
    for (uint32_t seg = gw; seg < a.numSegments; seg += totalWaves) {
        const uint32_t cnt = uniform(a.b.pathCnt[0][seg]), segBase = seg * a.segSize;
        for (uint32_t base = 0; base < cnt; base += 64) {
            if (base + lane >= cnt) continue;
            const uint32_t slot = segBase + base + lane;
            const float4 o = a.b.rayO[0][slot], d = a.b.rayD[0][slot], ha = a.b.hit[slot];
            const uint32_t smp = reinterpret_cast<const uint32_t*>(a.b.thr[0] + slot)[3];       // one accumulation index: sample == padded pixel
            const uint32_t tile = smp >> 6, within = smp & 63u;
            const bool columnMajor = a.rect.stripeCount > 1u;                                    // tile_position with selects, as in wf_gbuffer
            const uint32_t den = columnMajor ? a.tilesY : a.tilesX, quo = tile / den, rem = tile - quo * den;
            const uint32_t tcol = columnMajor ? quo : rem, trow = columnMajor ? rem : quo;
            const uint32_t px = a.rect.column_x(tcol) + (within & 7u), py = a.rect.y0 + trow * 8u + (within >> 3);
            const size_t idx = (size_t)py * a.imageWidth + px;
            uint32_t tri = __float_as_uint(ha.w);
            float4 texel[kGbPlanes];
            float4 motion = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (tri != 0xFFFFFFFFu) {
                tri &= 0x1FFFFFFFu;                                  // bits 29-31: shading class (wf_extend)
                Hit h; h.valid = true; h.t = ha.x; h.u = ha.y; h.v = ha.z; h.tri = tri; h.prim = 0; h.inst = s.instances ? a.b.hitInst[slot] : 0u; h.opaque = 1;
                const MotionTri mt = motion_gather(s, m, h);
                if constexpr (PLANES) {
                    Ray ray; ray.o = mk3(o.x, o.y, o.z); ray.d = mk3(d.x, d.y, d.z); ray.tmin = o.w; ray.tmax = 1e10f;
                    gbuffer_texels(s, cb, ray, h, texel);
                }
                motion = motion_texel(cb.m_View, m, mt, h.u, h.v);
            } else if constexpr (PLANES) gbuffer_miss(texel);
            if constexpr (PLANES) gbuffer_store(g, planeMask, idx, texel);
            m.plane[idx] = motion;
        }
    }
}
