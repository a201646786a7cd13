// ygzf_api_remap.hip -- the undistortion in front of ORBextractor::ComputePyramid: cv::remap(mImGray, ..., map1, map2, cv::INTER_LINEAR) of
// Frame::ComputeImagePyramid (src/Frame.cc:775-805) as entry points of the C ABI (include/ygzf.h states the arithmetic and the rules).  Product code.
// The plan of a map is host arithmetic (ygzf_remap_plan.hip), the kernels are remap_kernels.hip; this file owns ygzf_ctx::remap.
#include "ygzf_ctx.h"

typedef ygzf_ctx::Remap::Map RemapMap;

static int map_of(ygzf_ctx *c, int map_id, RemapMap **m) {
    if (map_id < 0 || map_id >= kRemapMaps) return fail(c, YGZF_ERR_INVALID, "map_id %d (0 or 1: one per eye)", map_id);
    *m = &c->remap.map[map_id];
    if (!(*m)->set) return fail(c, YGZF_ERR_STATE, "no map set for id %d (ygzf_remap_set)", map_id);
    return YGZF_OK;
}

// src/Frame.cc:775-805: the maps of cv::initUndistortRectifyMap, planned on the host and uploaded
int ygzf_remap_set(ygzf_ctx *c, int map_id, int src_w, int src_h, int w, int h, const int16_t *map_xy, const uint16_t *map_tab) {
    if (!c) return YGZF_ERR_INVALID;
    if (map_id < 0 || map_id >= kRemapMaps) return fail(c, YGZF_ERR_INVALID, "map_id %d (0 or 1: one per eye)", map_id);
    if (!map_xy || !map_tab) return fail(c, YGZF_ERR_INVALID, "null map");
    if (src_w < 1 || src_h < 1 || w < 1 || h < 1 || src_w > c->maxW || src_h > c->maxH || w > c->maxW || h > c->maxH)
        return fail(c, YGZF_ERR_INVALID, "map %dx%d -> %dx%d beyond the context's %dx%d", src_w, src_h, w, h, c->maxW, c->maxH);
    RemapPlan P;
    std::string msg;
    int rc = build_remap_plan(src_w, src_h, w, h, map_xy, map_tab, P, &msg);
    if (rc) return fail(c, rc, "%s", msg.c_str());
    // Workgroups are dealt round-robin over the eight XCDs, so list positions p and p + 8 run on one XCD at about the same time: the staged
    // tiles are listed so that those are neighbours.  A tile row is 64 bytes of a 128-byte line whose other half belongs to the tile beside it --
    // one XCD's L2 then sees both halves, of the source lines it fetches and of the destination lines it writes back (256 frames at 752 x 480:
    // 91 against 100 us).  The gathered tiles keep the plan's order: the same listing cost k_remap_gather a tenth (322 against 292 us).
    if (c->remap.xcdOrder) {
        const std::vector<int> in = P.listStaged;
        const size_t n = in.size(), per = (n + 7) / 8;
        size_t p = 0;
        for (size_t i = 0; i < per; i++)
            for (size_t k = 0; k < 8; k++)
                if (k * per + i < n) P.listStaged[p++] = in[k * per + i];
    }
    HIPCHECK(c, hipSetDevice(c->device));
    // the new tables are built beside the old ones and moved in at the end: an error on the way leaves the id's previous map working
    RemapMap M;
    const size_t nPx = P.rec.size() * sizeof(uint32_t), nT = P.tiles.size() * sizeof(RemapTileRec);
    if ((rc = ensure(c, M.rec, nPx)) || (rc = ensure(c, M.xy, nPx)) || (rc = ensure(c, M.tiles, nT)) ||
        (rc = ensure(c, M.listStaged, sizeof(int) * std::max<size_t>(P.listStaged.size(), 1))) ||
        (rc = ensure(c, M.listGather, sizeof(int) * std::max<size_t>(P.listGather.size(), 1))))
        return rc;
    HIPCHECK(c, hipMemcpyAsync(M.rec.p, P.rec.data(), nPx, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(c, hipMemcpyAsync(M.xy.p, P.xy.data(), nPx, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(c, hipMemcpyAsync(M.tiles.p, P.tiles.data(), nT, hipMemcpyHostToDevice, c->stream));
    if (!P.listStaged.empty()) HIPCHECK(c, hipMemcpyAsync(M.listStaged.p, P.listStaged.data(), sizeof(int) * P.listStaged.size(), hipMemcpyHostToDevice, c->stream));
    if (!P.listGather.empty()) HIPCHECK(c, hipMemcpyAsync(M.listGather.p, P.listGather.data(), sizeof(int) * P.listGather.size(), hipMemcpyHostToDevice, c->stream));
    // (the plan's vectors leave with this call, and a queued remap may still read the tables about to be replaced)
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    M.set = true;
    M.srcW = src_w; M.srcH = src_h; M.w = w; M.h = h;
    M.recPitch = P.recPitch; M.tilesX = P.tilesX; M.tilesY = P.tilesY;
    M.nStaged = (int) P.listStaged.size(); M.nGather = (int) P.listGather.size();
    for (int k = 0; k < 4; k++) M.count[k] = P.count[k];
    c->remap.map[map_id] = std::move(M);
    return YGZF_OK;
}

int ygzf_remap_clear(ygzf_ctx *c, int map_id) {
    if (!c) return YGZF_ERR_INVALID;
    if (map_id < 0 || map_id >= kRemapMaps) return fail(c, YGZF_ERR_INVALID, "map_id %d (0 or 1: one per eye)", map_id);
    HIPCHECK(c, hipSetDevice(c->device));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    c->remap.map[map_id] = RemapMap();
    return YGZF_OK;
}

int ygzf_remap_info(const ygzf_ctx *c_, int map_id, int *info) {
    ygzf_ctx *c = const_cast<ygzf_ctx *>(c_);
    if (!c || !info) return fail(c, YGZF_ERR_INVALID, "null argument");
    RemapMap *m;
    int rc = map_of(c, map_id, &m);
    if (rc) return rc;
    const int v[9] = {m->srcW, m->srcH, m->w, m->h, m->count[0], m->count[1], m->count[2], m->count[3], c->remap.framesPerRun};
    memcpy(info, v, sizeof v);
    return YGZF_OK;
}

int ygzf_remap_set_path(ygzf_ctx *c, int path) {
    if (!c) return YGZF_ERR_INVALID;
    if (path != YGZF_REMAP_PATH_AUTO && path != YGZF_REMAP_PATH_LDS && path != YGZF_REMAP_PATH_GATHER) return fail(c, YGZF_ERR_INVALID, "remap path %d", path);
    c->remap.path = path;
    return YGZF_OK;
}

int ygzf_remap_stats(const ygzf_ctx *c, int *stats) {
    if (!c || !stats) return YGZF_ERR_INVALID;
    memcpy(stats, c->remap.stats, sizeof c->remap.stats);
    return YGZF_OK;
}

// Queues the remap of n frames on the context's stream.  AUTO is LDS: on the EuRoC map staging takes a third of the gather kernel's time
// (profiles/remap_rate.txt); GATHER sends every tile -- the Empty ones included -- through k_remap_gather.
static int queue_remap(ygzf_ctx *c, const RemapMap &m, const uint8_t *src, int n, long long srcPitch, long long srcStride, uint8_t *dst, long long dstPitch,
                       long long dstStride) {
    RemapArgs A;
    A.rec = (const uint32_t *) m.rec.p;
    A.xy = (const uint32_t *) m.xy.p;
    A.tiles = (const RemapTileRec *) m.tiles.p;
    A.list = nullptr;
    A.w = m.w; A.h = m.h; A.recPitch = m.recPitch; A.tilesX = m.tilesX; A.srcW = m.srcW; A.srcH = m.srcH;
    A.src = src; A.srcPitch = srcPitch; A.srcStride = srcStride;
    A.dst = dst; A.dstPitch = dstPitch; A.dstStride = dstStride;
    A.nFrames = n;
    A.framesPerRun = std::max(1, c->remap.framesPerRun);
    A.srcAligned = (((uintptr_t) src | (unsigned long long) srcPitch | (unsigned long long) srcStride) & 3) == 0;
    A.dstAligned = (((uintptr_t) dst | (unsigned long long) dstPitch | (unsigned long long) dstStride) & 3) == 0;
    int *S = c->remap.stats;
    S[0] = S[1] = S[2] = 0;
    S[3] = (n + A.framesPerRun - 1) / A.framesPerRun;
    if (c->remap.path == YGZF_REMAP_PATH_GATHER) {
        S[2] = m.tilesX * m.tilesY;
        launch_remap_gather(c->stream, A, S[2]);   // (no list: tile i)
    } else {
        S[0] = m.count[kRemapInside] + m.count[kRemapLds];
        S[1] = m.count[kRemapEmpty];
        S[2] = m.nGather;
        A.list = (const int *) m.listStaged.p;
        launch_remap_tiles(c->stream, A, m.nStaged);
        A.list = (const int *) m.listGather.p;
        launch_remap_gather(c->stream, A, m.nGather);
    }
    HIPCHECK(c, hipGetLastError());
    return YGZF_OK;
}

// src/Frame.cc:775-805 for frames that already lie in device memory: the output is what ygzf_extract_batch_device takes
int ygzf_remap_batch_device(ygzf_ctx *c, int map_id, const uint8_t *d_src, int n_frames, int src_row_pitch, size_t src_frame_stride, uint8_t *d_dst,
                            int dst_row_pitch, size_t dst_frame_stride) {
    if (!c || !d_src || !d_dst) return fail(c, YGZF_ERR_INVALID, "null argument");
    RemapMap *m;
    int rc = map_of(c, map_id, &m);
    if (rc) return rc;
    if (n_frames < 1 || n_frames > 65535 * std::max(1, c->remap.framesPerRun)) return fail(c, YGZF_ERR_INVALID, "n_frames %d", n_frames);
    if (src_row_pitch < m->srcW || dst_row_pitch < m->w) return fail(c, YGZF_ERR_INVALID, "row pitch below the width (source %d < %d or destination %d < %d)", src_row_pitch, m->srcW, dst_row_pitch, m->w);
    if (n_frames > 1 && (src_frame_stride < (size_t) src_row_pitch * (m->srcH - 1) + m->srcW || dst_frame_stride < (size_t) dst_row_pitch * (m->h - 1) + m->w))
        return fail(c, YGZF_ERR_INVALID, "frame stride below the frame's bytes");
    HIPCHECK(c, hipSetDevice(c->device));
    return queue_remap(c, *m, d_src, n_frames, src_row_pitch, (long long) src_frame_stride, d_dst, dst_row_pitch, (long long) dst_frame_stride);
}

// the raw image into remap.in, tight (one linear copy where the caller's rows are tight as well)
static int upload_raw(ygzf_ctx *c, const RemapMap &m, const uint8_t *src, int stride) {
    int rc = ensure(c, c->remap.in, (size_t) m.srcW * m.srcH);
    if (rc) return rc;
    if (stride == m.srcW) HIPCHECK(c, hipMemcpyAsync(c->remap.in.p, src, (size_t) m.srcW * m.srcH, hipMemcpyHostToDevice, c->stream));
    else HIPCHECK(c, hipMemcpy2DAsync(c->remap.in.p, (size_t) m.srcW, src, (size_t) stride, (size_t) m.srcW, (size_t) m.srcH, hipMemcpyHostToDevice, c->stream));
    return YGZF_OK;
}

// src/Frame.cc:792-797: the right eye's image, host to host
int ygzf_remap_host(ygzf_ctx *c, int map_id, const uint8_t *src, int src_stride, uint8_t *dst, int dst_stride) {
    if (!c || !src || !dst) return fail(c, YGZF_ERR_INVALID, "null argument");
    RemapMap *m;
    int rc = map_of(c, map_id, &m);
    if (rc) return rc;
    if (src_stride < m->srcW || dst_stride < m->w) return fail(c, YGZF_ERR_INVALID, "stride below the width");
    HIPCHECK(c, hipSetDevice(c->device));
    if ((rc = upload_raw(c, *m, src, src_stride)) || (rc = ensure(c, c->remap.out, (size_t) m->w * m->h))) return rc;
    if ((rc = queue_remap(c, *m, (const uint8_t *) c->remap.in.p, 1, m->srcW, 0, (uint8_t *) c->remap.out.p, m->w, 0))) return rc;
    if (dst_stride == m->w) HIPCHECK(c, hipMemcpyAsync(dst, c->remap.out.p, (size_t) m->w * m->h, hipMemcpyDeviceToHost, c->stream));
    else HIPCHECK(c, hipMemcpy2DAsync(dst, (size_t) dst_stride, c->remap.out.p, (size_t) m->w, (size_t) m->w, (size_t) m->h, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return YGZF_OK;
}

// src/Frame.cc:775-813: undistort, then ORBextractor::ComputePyramid of the undistorted image -- ygzf_compute_pyramid with the remap in the place
// of the upload's last step: the raw image crosses the link once, level 0 is written by the remap kernel at the context's pitch
int ygzf_compute_pyramid_remapped(ygzf_ctx *c, int map_id, const uint8_t *img, int stride, uint8_t *const *levels_out) {
    if (!c || !img || !levels_out) return fail(c, YGZF_ERR_INVALID, "null argument");
    RemapMap *m;
    int rc = map_of(c, map_id, &m);
    if (rc) return rc;
    if (stride < m->srcW) return fail(c, YGZF_ERR_INVALID, "stride %d < width %d", stride, m->srcW);
    HIPCHECK(c, hipSetDevice(c->device));
    const int w = m->w, h = m->h;
    if ((rc = apply_geometry(c, w, h, 1))) return rc;
    if (c->extractAhead && c->streamCopy && (rc = save_carry_pyramid(c))) return rc;   // (as ygzf_compute_pyramid: before dPyr is written over)
    if ((rc = upload_raw(c, *m, img, stride))) return rc;
    forget_image(c);
    if ((rc = ensure(c, c->dImg0, (size_t) align_up(w, 64) * h))) return rc;
    const FrameSet fs = own_frames(c, w, h);
    if ((rc = queue_remap(c, *m, (const uint8_t *) c->remap.in.p, 1, m->srcW, 0, (uint8_t *) c->dImg0.p, fs.img0_pitch, 0))) return rc;
    return pyramid_readback(c, fs, w, h, nullptr, 0, levels_out);
}
