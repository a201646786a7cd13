// ygzf_api_match.hip -- ORBmatcher's entry points: SearchByProjection (all overloads), SearchByBoW, SearchForInitialization, SearchForTriangulation, Fuse (candidate search), the Frame grid, Frame::isInFrustum, MapPoint::ComputeDistinctiveDescriptors, ORBVocabulary::transform (C ABI of libygzf, include/ygzf.h; product code: no CPU fallback, nothing from oracle/ is included or linked).
#include "ygzf_ctx.h"

extern "C" {

// ---- matcher ----------------------------------------------------------------------------------------------------------
static void grid_inverses(const ygzf_camera &cam, float &invW, float &invH) {   // mfGridElementWidthInv / HeightInv, src/Frame.cc:302-303
    invW = (float) 64 / (cam.max_x - cam.min_x);
    invH = (float) 48 / (cam.max_y - cam.min_y);
}

static void fill_camera(MatchArgs &A, const ygzf_camera *cam, const ygzf_ctx *c) {
    A.fx = cam->fx; A.fy = cam->fy; A.cx = cam->cx; A.cy = cam->cy; A.mb = cam->mb; A.mbf = cam->mbf;
    A.minX = cam->min_x; A.minY = cam->min_y; A.maxX = cam->max_x; A.maxY = cam->max_y;
    grid_inverses(*cam, A.gridInvW, A.gridInvH);
    for (int l = 0; l < kMaxLevels; l++) A.scaleFactors[l] = l < c->tab.cfg.nlevels ? c->tab.scale[l] : 1.f;
}
// ... and the caller's own scale factors, where a frame view brings them, over the context's
static void fill_view_scales(MatchArgs &A, const ygzf_frame_view *F) {
    if (F->scale_factors) for (int l = 0; l < kMaxLevels && l < F->nlevels; l++) A.scaleFactors[l] = F->scale_factors[l];
}

static int plan_match_lds(ygzf_ctx *c, MatchArgs &A, int nPairs, size_t *ldsBytes) {
    if (A.capCur > 65535) return fail(c, YGZF_ERR_UNSUPPORTED, "matcher supports at most 65535 keypoints per frame");
    A.qpInLds = 0;
    size_t b = 0, sp = 0;
    bool ok = false;
    for (const MatchLdsPlan &pl : kMatchLdsPlans) {   // in order of preference (lds_layout.h)
        const MatchLdsBytes need = match_lds_bytes(A.capCur, A.capLast, pl.desc != 0, pl.spill, A.specDeep != 0);
        b = need.lds;
        sp = need.spill;
        if (b <= kMatchLdsBudget) { A.descInLds = pl.desc; A.spill = pl.spill; ok = true; break; }
    }
    if (!ok) return fail(c, YGZF_ERR_UNSUPPORTED, "matcher needs %zu bytes of LDS for %d/%d keypoints", b, A.capCur, A.capLast);
    int rc = ensure(c, c->dQp, (size_t) nPairs * A.capLast * 32);
    if (rc) return rc;
    A.qpScratch = c->dQp.p;
    A.spillStride = (long long) sp;
    A.spillScratch = nullptr;
    if (sp) {
        if ((rc = ensure(c, c->dSpill, (size_t) nPairs * sp))) return rc;
        A.spillScratch = c->dSpill.p;
    }
    // few pairs in the launch (a Tracking thread matches ONE): spread each over several workgroups (kernels.h, MatchArgs::split)
    if (!c->dMatchStat.p) {
        if ((rc = ensure(c, c->dMatchStat, 64))) return rc;
        HIPCHECK(c, hipMemsetAsync(c->dMatchStat.p, 0, 64, c->stream));
    }
    A.matchStat = (unsigned *) c->dMatchStat.p;
    A.serialOrder = c->matchSerial;
    A.handoverFence = c->matchFence;
    A.fixedLanes = c->matchFixedLanes;
    A.scanFiltered = c->matchScanFiltered;
    A.split = 1;
    A.splitCnt = nullptr;
    A.splitX = nullptr;
    if (!A.spill && A.capLast >= 128 && c->matchSplit != 1) {
        int sp2 = c->matchSplit > 1 ? c->matchSplit : 256 / (nPairs > 0 ? nPairs : 1);
        sp2 = std::min(sp2, c->matchSplit > 1 ? 128 : 64);   // (one pair: 64 workgroups of 16 queries, four waves each in the scan: 35.5 us against 41.7 at 8)
        if (sp2 > 1) {
            const size_t cntBytes = (size_t) nPairs * sizeof(int);
            if (c->dSplitCnt.bytes < cntBytes) {   // counters are zero between launches: a fresh buffer is cleared once
                if ((rc = ensure(c, c->dSplitCnt, cntBytes > 4096 ? cntBytes : 4096))) return rc;
                HIPCHECK(c, hipMemsetAsync(c->dSplitCnt.p, 0, c->dSplitCnt.bytes, c->stream));
            }
            if ((rc = ensure(c, c->dSplitX, (size_t) nPairs * A.capLast * kMatchSplitRec))) return rc;
            A.split = sp2;
            A.splitCnt = (int *) c->dSplitCnt.p;
            A.splitX = (unsigned char *) c->dSplitX.p;
        }
    }
    HIPCHECK(c, match_prepare(b));
    *ldsBytes = b;
    return YGZF_OK;
}

// The k_match_last launch of every entry point below, from a filled MatchArgs.  Under YGZF_DEBUG=match the phase stamps of pair `dbgPair` go to
// stderr (a blocking copy of their own, so the caller's download may come after).
static int run_match(ygzf_ctx *c, MatchArgs &A, int nPairs, int dbgPair, const char *label) {
    int rc;
    if (c->matchDebug) {
        if ((rc = ensure(c, c->dMatchClk, (size_t) nPairs * 8 * sizeof(long long)))) return rc;
        A.dbg = (long long *) c->dMatchClk.p;
    }
    size_t lds;
    if ((rc = plan_match_lds(c, A, nPairs, &lds))) return rc;
    {
        ProfScope ps(c, KK_MATCH);
        launch_match_last(c->stream, A, nPairs, lds);
    }
    HIPCHECK(c, hipGetLastError());
    if (A.dbg) {
        long long st[8];
        HIPCHECK(c, hipMemcpy(st, A.dbg + 8 * dbgPair, sizeof st, hipMemcpyDeviceToHost));
        fprintf(stderr, "[ygzf match %s, 100MHz ticks] grid %lld  proj %lld  spec %lld  seq %lld  tail %lld  rescans %lld of %lld queries\n", label,
                st[1] - st[0], st[2] - st[1], st[3] - st[2], st[4] - st[3], st[5] - st[4], st[6], st[7]);
    }
    return YGZF_OK;
}

// One (Cur, Last) pair whose arrays ride the caller's PackedTransfer: Cur's keys / descriptors / mvuRight / owners, the two counts and the three
// outputs.  add() before P.upload(), fill() after it.  A null ownerOut / matchOut keeps that output on the device (kernel scratch).
struct PackedPair {
    const ygzf_frame_view *F;
    int counts[2];
    size_t keys, desc, uRight, ownerIn, cnt, owner, match, nmatches;
    void add(PackedTransfer &P, const ygzf_frame_view *F_, int nLast, const uint8_t *ownerIn_, uint8_t *ownerOut, int *matchOut, int *nmatchesOut) {
        F = F_;
        counts[0] = F->n; counts[1] = nLast;
        const size_t nt = (size_t) F->n;
        keys = P.add_in(F->keys, nt * sizeof(ygzf_kp));
        desc = P.add_in(F->desc, nt * 32);
        uRight = P.add_in(F->u_right, F->u_right ? nt * 4 : 0);
        ownerIn = P.add_in(ownerIn_, nt);
        cnt = P.add_in(counts, sizeof counts);
        owner = P.add_out(ownerOut, nt);
        match = P.add_out(matchOut, nt * sizeof(int));
        nmatches = P.add_out(nmatchesOut, sizeof(int));
    }
    void fill(MatchArgs &A, const PackedTransfer &P, const uint8_t *dIn) const {
        A.curKeys = (const ygzf_kp *) (dIn + keys);
        A.curDesc = dIn + desc;
        A.curURight = F->u_right ? (const float *) (dIn + uRight) : nullptr;
        A.ownerIn = dIn + ownerIn;
        A.curCnt = A.lastCnt = (const int *) (dIn + cnt);   // one pair: count strides 0, Cur's count first
        A.cntStrideCur = A.cntStrideLast = 0;
        A.cntOffCur = 0;
        A.cntOffLast = 1;
        A.kpStrideCur = A.capCur = counts[0];
        A.kpStrideLast = A.capLast = counts[1];
        A.owner = P.d_out(owner);
        A.match = (int *) P.d_out(match);
        A.nmatches = (int *) P.d_out(nmatches);
    }
};

int ygzf_match_batch_prev(ygzf_ctx *c, const ygzf_camera *cam, float th, int b_mono, int check_level, int check_orientation) {
    if (!c || !cam) return fail(c, YGZF_ERR_INVALID, "null argument");
    int rc = need_carried_batch(c);
    if (rc) return rc;
    HIPCHECK(c, hipSetDevice(c->device));
    const Geometry &G = c->geo;
    const int B = c->held.frames;
    if (G.kpStride == 0) return fail(c, YGZF_ERR_STATE, "configuration yields no keypoints");
    if ((rc = ensure(c, c->dWorld, (size_t) (B + 1) * G.kpStride * 3 * sizeof(float))) ||
        (rc = ensure(c, c->dOwner, (size_t) B * G.kpStride)) || (rc = ensure(c, c->dMatch, (size_t) B * G.kpStride * sizeof(int))) ||
        (rc = ensure(c, c->dNMatch, (size_t) B * sizeof(int))) || (rc = ensure(c, c->dPoses, (size_t) B * 24 * sizeof(float))))
        return rc;
    // identity poses for every pair (uploaded once per buffer / batch size, so the steady state has no host sync)
    if (c->identityPoses < B || c->identityPosesPtr != c->dPoses.p) {
        std::vector<float> poses((size_t) B * 24, 0.f);
        for (int p = 0; p < B; p++) {
            float *q = &poses[(size_t) p * 24];
            q[0] = q[4] = q[8] = 1.f;
            q[12] = q[16] = q[20] = 1.f;
        }
        HIPCHECK(c, hipMemcpyAsync(c->dPoses.p, poses.data(), poses.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHECK(c, hipStreamSynchronize(c->stream));  // `poses` goes out of scope
        c->identityPoses = B;
        c->identityPosesPtr = c->dPoses.p;
    }
    const ygzf_kp *kp = (const ygzf_kp *) c->dOutKp.p;
    const uint8_t *desc = (const uint8_t *) c->dOutDesc.p;
    const int *cnt = (const int *) c->dOutCnt.p;
    MatchArgs A;
    memset(&A, 0, sizeof A);
    A.maxDist = 100;   // TH_HIGH
    A.unitWorld = 1;   // world point of a Last keypoint = its back-projection to depth 1, computed where it is used (a launch of its own until round 4)
    A.curKeys = kp + G.kpStride;            // pair p: Cur = slot p+1, Last = slot p
    A.curDesc = desc + (size_t) G.kpStride * 32;
    A.curURight = nullptr;
    A.curCnt = cnt;
    A.kpStrideCur = G.kpStride;
    A.cntStrideCur = 1;
    A.cntOffCur = 1;
    A.ownerIn = nullptr;
    A.lastKeys = kp;
    A.mpDesc = desc;
    A.world = (const float *) c->dWorld.p;
    A.lastCnt = cnt;
    A.kpStrideLast = G.kpStride;
    A.cntStrideLast = 1;
    A.cntOffLast = 0;
    A.poses = (const float *) c->dPoses.p;
    fill_camera(A, cam, c);
    A.th = th;
    A.bMono = b_mono != 0;
    A.checkLevel = check_level != 0;
    A.checkOri = check_orientation != 0;
    A.owner = (uint8_t *) c->dOwner.p;
    A.match = (int *) c->dMatch.p;
    A.nmatches = (int *) c->dNMatch.p;
    A.capCur = G.kpStride;
    A.capLast = G.kpStride;
    if ((rc = run_match(c, A, B, B > 1 ? 1 : 0, B > 1 ? "pair 1" : "pair 0"))) return rc;
    set_match_pairs(c, B);
    return YGZF_OK;
}

static int read_match_stats(ygzf_ctx *c, unsigned *dst, int words) {
    if (!c || !dst) return fail(c, YGZF_ERR_INVALID, "null argument");
    for (int i = 0; i < words; i++) dst[i] = 0;
    if (!c->dMatchStat.p) return YGZF_OK;   // no matcher launch yet
    HIPCHECK(c, hipSetDevice(c->device));
    HIPCHECK(c, hipMemcpyAsync(dst, c->dMatchStat.p, words * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return YGZF_OK;
}
int ygzf_match_fallbacks(ygzf_ctx *c, unsigned *pairs) { return read_match_stats(c, pairs, 1); }
int ygzf_match_path_stats(ygzf_ctx *c, unsigned stats[5]) { return read_match_stats(c, stats, kMatchStatWords); }

int ygzf_match_counts(ygzf_ctx *c, int *nmatches) {
    if (!c || !nmatches) return fail(c, YGZF_ERR_INVALID, "null argument");
    if (c->held.matchPairs < 1) return fail(c, YGZF_ERR_STATE, "no matched batch");
    HIPCHECK(c, hipMemcpyAsync(nmatches, c->dNMatch.p, sizeof(int) * c->held.matchPairs, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return YGZF_OK;
}

int ygzf_match_fetch(ygzf_ctx *c, int frame, int *cur_match, uint8_t *cur_owner, int cap) {
    if (!c) return fail(c, YGZF_ERR_INVALID, "null argument");
    if (c->held.matchPairs < 1) return fail(c, YGZF_ERR_STATE, "no matched batch");
    if (frame < 0 || frame >= c->held.matchPairs) return fail(c, YGZF_ERR_INVALID, "frame %d out of range", frame);
    int n = 0;
    HIPCHECK(c, hipMemcpyAsync(&n, (int *) c->dOutCnt.p + frame + 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    if (n > cap) return fail(c, YGZF_ERR_INVALID, "capacity %d < %d keypoints", cap, n);
    const size_t base = (size_t) frame * c->geo.kpStride;
    if (cur_match && n) HIPCHECK(c, hipMemcpyAsync(cur_match, (int *) c->dMatch.p + base, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
    if (cur_owner && n) HIPCHECK(c, hipMemcpyAsync(cur_owner, (uint8_t *) c->dOwner.p + base, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return YGZF_OK;
}

int ygzf_match_fetch_all(ygzf_ctx *c, int *match, int stride) {
    if (!c || !match) return fail(c, YGZF_ERR_INVALID, "null argument");
    if (c->held.matchPairs < 1) return fail(c, YGZF_ERR_STATE, "no matched batch");
    const int B = c->held.matchPairs, ks = c->geo.kpStride;
    if (stride < ks) return fail(c, YGZF_ERR_INVALID, "stride %d < %d (ygzf_max_keypoints)", stride, ks);
    HIPCHECK(c, hipMemcpy2DAsync(match, sizeof(int) * (size_t) stride, c->dMatch.p, sizeof(int) * (size_t) ks, sizeof(int) * (size_t) ks, B,
                                 hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return YGZF_OK;
}

int ygzf_search_by_projection_last(ygzf_ctx *c, const ygzf_frame_view *cur, const ygzf_camera *cam, int last_n, const ygzf_kp *last_keys,
                                   const uint8_t *mp_valid, const uint8_t *outlier, const uint8_t *mp_has_obs, const float *mp_world,
                                   const uint8_t *mp_desc, const float *Rcw, const float *tcw, const float *Rlw, const float *tlw, float th,
                                   int b_mono, int check_level, int check_orientation, uint8_t *cur_owner, int *cur_match, int *nmatches) {
    if (!c || !cur || !cam || !nmatches || !Rcw || !tcw || !Rlw || !tlw) return fail(c, YGZF_ERR_INVALID, "null argument");
    *nmatches = 0;
    if (cur->n < 0 || last_n < 0) return fail(c, YGZF_ERR_INVALID, "negative count");
    if (cur->n == 0 || last_n == 0) {
        for (int i = 0; i < cur->n; i++) if (cur_match) cur_match[i] = -1;
        return YGZF_OK;
    }
    if (!cur->keys || !cur->desc || !last_keys || !mp_world || !mp_desc || !cur_match || !cur_owner)
        return fail(c, YGZF_ERR_INVALID, "null array");
    {   // the kernel indexes its scale-factor table with these octaves and stores Cur's as bytes
        const int nl = cur->scale_factors ? std::min(cur->nlevels, (int) kMaxLevels) : c->tab.cfg.nlevels;
        for (int i = 0; i < last_n; i++)
            if (last_keys[i].octave < 0 || last_keys[i].octave >= nl) return fail(c, YGZF_ERR_INVALID, "last_keys[%d].octave %d outside 0..%d", i, last_keys[i].octave, nl - 1);
        for (int i = 0; i < cur->n; i++)
            if (cur->keys[i].octave < 0 || cur->keys[i].octave >= nl) return fail(c, YGZF_ERR_INVALID, "cur keys[%d].octave %d outside 0..%d", i, cur->keys[i].octave, nl - 1);
    }
    HIPCHECK(c, hipSetDevice(c->device));
    const size_t nq = last_n;
    float pose[24];
    memcpy(pose, Rcw, 36); memcpy(pose + 9, tcw, 12); memcpy(pose + 12, Rlw, 36); memcpy(pose + 21, tlw, 12);
    PackedTransfer P(c);
    PackedPair pair;
    pair.add(P, cur, last_n, cur_owner, cur_owner, cur_match, nmatches);
    const size_t oLastK = P.add_in(last_keys, nq * sizeof(ygzf_kp)), oMpD = P.add_in(mp_desc, nq * 32), oWorld = P.add_in(mp_world, nq * 12),
                 oValid = P.add_in(mp_valid, mp_valid ? nq : 0), oOutl = P.add_in(outlier, outlier ? nq : 0),
                 oObs = P.add_in(mp_has_obs, mp_has_obs ? nq : 0), oPose = P.add_in(pose, sizeof pose);
    int rc;
    uint8_t *dIn;
    if ((rc = P.upload(&dIn))) return rc;
    MatchArgs A;
    memset(&A, 0, sizeof A);
    A.maxDist = 100;   // TH_HIGH
    pair.fill(A, P, dIn);
    A.lastKeys = (const ygzf_kp *) (dIn + oLastK);
    A.mpDesc = dIn + oMpD;
    A.world = (const float *) (dIn + oWorld);
    A.mpValid = mp_valid ? dIn + oValid : nullptr;
    A.outlier = outlier ? dIn + oOutl : nullptr;
    A.hasObs = mp_has_obs ? dIn + oObs : nullptr;
    A.poses = (const float *) (dIn + oPose);
    fill_camera(A, cam, c);
    fill_view_scales(A, cur);
    A.th = th;
    A.bMono = b_mono != 0;
    A.checkLevel = check_level != 0;
    A.checkOri = check_orientation != 0;
    if ((rc = run_match(c, A, 1, 0, "(cur, last)")) || (rc = P.download())) return rc;
    set_match_pairs(c, 0);
    return YGZF_OK;
}

// MapPoint::PredictScale (src/MapPoint.cc:359-373) is a non-decreasing step function of ratio = mfMaxDistance / dist; its steps are
// tabulated here with the host's own libm so that the device reproduces it by comparisons: step[k] = smallest float ratio whose level
// is >= k (k = 1 .. nlevels-1).
static int predict_scale_host(float ratio, float logScaleFactor, int nScaleLevels) {
    int nScale = (int) std::ceil(std::log(ratio) / logScaleFactor);
    if (nScale < 0) nScale = 0;
    else if (nScale >= nScaleLevels) nScale = nScaleLevels - 1;
    return nScale;
}
static void predict_scale_steps(float logScaleFactor, int nScaleLevels, float *step) {
    for (int k = 0; k < kMaxLevels; k++) step[k] = std::numeric_limits<float>::infinity();
    for (int k = 1; k < nScaleLevels && k < kMaxLevels; k++) {
        uint32_t lo = 0x00800000u, hi = 0x7F7FFFFFu;   // positive normal floats, ordered like their bit patterns
        auto lvl = [&](uint32_t b) { float r; memcpy(&r, &b, 4); return predict_scale_host(r, logScaleFactor, nScaleLevels); };
        if (lvl(hi) < k) continue;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (lvl(mid) >= k) hi = mid; else lo = mid + 1;
        }
        memcpy(&step[k], &lo, 4);
    }
}

struct FrustumHost {   // host-side inputs of the fused isInFrustum stage (ygzf_frustum_in without the ABI wrapper)
    const ygzf_frustum_in *in;
    uint8_t *in_view;
    float *proj_x, *proj_y, *proj_xr, *view_cos;
    int *level;
};

struct ProjectedQuery {   // projected_match's queries, thresholds and outputs; zero / null: absent
    int mode;             // 1: F x local MapPoints, 2: Cur x KeyFrame points, 3: SearchForInitialization's window search
    int n_mp;
    const uint8_t *track_in_view, *is_bad, *mp_has_obs;
    const float *proj_x, *proj_y, *proj_xr;
    const float *view_cos, *mp_angle;   // mode 1 / mode 2
    const int *scale_level;
    const uint8_t *mp_desc;
    float th, nnratio;
    int check_level, max_dist, check_ori;
    uint8_t *owner;
    int *match, *nmatches;
    const ygzf_kp *last_keys;   // mode 3
    int *match12;               // mode 3
    const FrustumHost *fr;      // mode 1: Frame::isInFrustum runs on the device first and supplies the projections
};

// The frustum inputs join the caller's packed upload (frustum_add_inputs before PackedTransfer::upload, frustum_fill_args after it).
struct FrustumOffsets { size_t world, normal, maxInv, minInv, mfMax, cand; };

static int frustum_add_inputs(ygzf_ctx *c, PackedTransfer &P, FrustumOffsets &O, const ygzf_frustum_in *in, int n, int nlevels) {
    if (!in->world || !in->normal || !in->max_dist_inv || !in->min_dist_inv || !in->mf_max_distance) return fail(c, YGZF_ERR_INVALID, "null frustum array");
    if (nlevels < 1 || nlevels > kMaxLevels) return fail(c, YGZF_ERR_INVALID, "nlevels out of range");
    O.world = P.add_in(in->world, 12 * (size_t) n);
    O.normal = P.add_in(in->normal, 12 * (size_t) n);
    O.maxInv = P.add_in(in->max_dist_inv, 4 * (size_t) n);
    O.minInv = P.add_in(in->min_dist_inv, 4 * (size_t) n);
    O.mfMax = P.add_in(in->mf_max_distance, 4 * (size_t) n);
    O.cand = P.add_in(in->candidate, in->candidate ? (size_t) n : 0);
    return YGZF_OK;
}

static void frustum_fill_args(FrustumArgs &A, const uint8_t *dIn, const FrustumOffsets &O, const ygzf_frustum_in *in, const ygzf_camera *cam, int n, int nlevels) {
    memset(&A, 0, sizeof A);
    A.n = n;
    A.candidate = in->candidate ? dIn + O.cand : nullptr;
    A.world = (const float *) (dIn + O.world);
    A.normal = (const float *) (dIn + O.normal);
    A.maxDistInv = (const float *) (dIn + O.maxInv);
    A.minDistInv = (const float *) (dIn + O.minInv);
    A.mfMaxDistance = (const float *) (dIn + O.mfMax);
    memcpy(A.Rcw, in->Rcw, 36);
    memcpy(A.tcw, in->tcw, 12);
    memcpy(A.Ow, in->Ow, 12);
    A.fx = cam->fx; A.fy = cam->fy; A.cx = cam->cx; A.cy = cam->cy; A.mbf = cam->mbf;
    A.minX = cam->min_x; A.minY = cam->min_y; A.maxX = cam->max_x; A.maxY = cam->max_y;
    A.viewingCosLimit = in->viewing_cos_limit;
    predict_scale_steps(in->log_scale_factor, nlevels, A.levelStep);
    A.nLevels = nlevels;
}

// shared body of the searches whose queries arrive already projected
static int projected_match(ygzf_ctx *c, const ygzf_frame_view *F, const ygzf_camera *cam, const ProjectedQuery &Q) {
    const int mode = Q.mode, n_mp = Q.n_mp;
    const FrustumHost *fr = Q.fr;
    if (!c || !F || !cam || !Q.nmatches) return fail(c, YGZF_ERR_INVALID, "null argument");
    *Q.nmatches = 0;
    if (F->n < 0 || n_mp < 0) return fail(c, YGZF_ERR_INVALID, "negative count");
    if (F->n == 0 || n_mp == 0) {
        for (int i = 0; i < F->n; i++) if (Q.match) Q.match[i] = -1;
        return YGZF_OK;
    }
    if (!F->keys || !F->desc || ((!Q.proj_x || !Q.proj_y) && !fr) || !Q.mp_desc || !Q.owner || !Q.match) return fail(c, YGZF_ERR_INVALID, "null array");
    if (fr) {
        if (mode != 1) return fail(c, YGZF_ERR_INVALID, "fused frustum stage only feeds SearchByProjection(F, MapPoints)");
    } else if (mode != 3) {
        if (!Q.track_in_view || (mode == 1 && !Q.view_cos) || (mode == 2 && !Q.mp_angle) || !Q.scale_level) return fail(c, YGZF_ERR_INVALID, "null array");
        for (int i = 0; i < n_mp; i++)
            if (Q.track_in_view[i] && (Q.scale_level[i] < 0 || Q.scale_level[i] >= kMaxLevels)) return fail(c, YGZF_ERR_INVALID, "scale level out of range");
    } else if (!Q.last_keys || !Q.match12) return fail(c, YGZF_ERR_INVALID, "null array");
    HIPCHECK(c, hipSetDevice(c->device));
    const size_t nq = n_mp;
    float pose[24] = {0};
    const int frLevels = F->nlevels > 0 ? F->nlevels : c->tab.cfg.nlevels;
    // one packed copy in, one out (PackedTransfer).  The per-MapPoint arrays the fused isInFrustum stage WRITES (projections, viewing cosine,
    // predicted level, in-view flag) live in the output half so that the caller's optional copies of them ride the same copy back.
    PackedTransfer P(c);
    PackedPair pair;   // mode 3 keeps owner / match as kernel scratch (the caller derives them from match12)
    pair.add(P, F, n_mp, Q.owner, mode == 3 ? nullptr : Q.owner, mode == 3 ? nullptr : Q.match, Q.nmatches);
    const size_t oLastK = P.add_in(Q.last_keys, Q.last_keys ? nq * sizeof(ygzf_kp) : 0), oMpD = P.add_in(Q.mp_desc, nq * 32),
                 oBad = P.add_in(Q.is_bad, Q.is_bad ? nq : 0), oObs = P.add_in(Q.mp_has_obs, Q.mp_has_obs ? nq : 0), oPose = P.add_in(pose, sizeof pose);
    size_t oPX = 0, oPY = 0, oPXR = 0, oVC = 0, oLv = 0, oTV = 0;
    size_t rPX = 0, rPY = 0, rPXR = 0, rVC = 0, rLv = 0, rTV = 0, rM12 = 0;
    FrustumOffsets FO;
    int rc;
    if (fr) {
        if ((rc = frustum_add_inputs(c, P, FO, fr->in, n_mp, frLevels))) return rc;
        rLv = P.add_out(fr->level, nq * 4);
        rTV = P.add_out(fr->in_view, nq);
        rPX = P.add_out(fr->proj_x, nq * 4);
        rPY = P.add_out(fr->proj_y, nq * 4);
        rPXR = P.add_out(fr->proj_xr, nq * 4);
        rVC = P.add_out(fr->view_cos, nq * 4);
    } else {
        oPX = P.add_in(Q.proj_x, nq * 4);
        oPY = P.add_in(Q.proj_y, nq * 4);
        oPXR = P.add_in(Q.proj_xr, Q.proj_xr ? nq * 4 : 0);
        if (mode != 3) {
            oTV = P.add_in(Q.track_in_view, nq);
            oVC = P.add_in(mode == 2 ? Q.mp_angle : Q.view_cos, nq * 4);
            oLv = P.add_in(Q.scale_level, nq * 4);
        }
    }
    if (mode == 3) rM12 = P.add_out(Q.match12, nq * sizeof(int));
    uint8_t *dIn;
    if ((rc = P.upload(&dIn))) return rc;
    const float *dPX, *dY, *dXR, *dVC;
    const int *dLv;
    const uint8_t *dTV;
    if (fr) {   // Frame::isInFrustum on the device: its outputs land where the matcher reads them
        FrustumArgs FA;
        frustum_fill_args(FA, dIn, FO, fr->in, cam, n_mp, frLevels);
        FA.inView = P.d_out(rTV);
        FA.projX = (float *) P.d_out(rPX);
        FA.projY = (float *) P.d_out(rPY);
        FA.projXR = (float *) P.d_out(rPXR);
        FA.viewCos = (float *) P.d_out(rVC);
        FA.level = (int *) P.d_out(rLv);
        {
            ProfScope ps(c, KK_FRUSTUM);
            launch_frustum(c->stream, FA);
        }
        dPX = FA.projX; dY = FA.projY; dXR = FA.projXR; dVC = FA.viewCos; dLv = FA.level; dTV = FA.inView;
    } else {
        dPX = (const float *) (dIn + oPX);
        dY = (const float *) (dIn + oPY);
        dXR = Q.proj_xr ? (const float *) (dIn + oPXR) : nullptr;
        dVC = (const float *) (dIn + oVC);     // unused in mode 3
        dLv = (const int *) (dIn + oLv);
        dTV = mode != 3 ? dIn + oTV : nullptr;
    }
    MatchArgs A;
    memset(&A, 0, sizeof A);
    A.mode = mode;
    A.specDeep = mode == 1 ? 1 : 0;   // best AND runner-up among the free candidates: lists of eight (match_kernels.hip)
    // accept threshold (TH_HIGH, ORBdist of mode 2).  A candidate becomes "best" only with dist < 256 (`int bestDist = 256 ... if (dist < bestDist)`,
    // src/ORBmatcher.cc:1413-1429), so a threshold of 256 or more accepts exactly what 255 accepts -- except that the reference then also "accepts" a
    // MapPoint without any free candidate and writes mvpMapPoints[-1] (:1431-1432, undefined; its callers pass 100 and 64).  Defined here, as in the
    // oracle, as: no candidate, no match.  (Found by the fuzzer once its KeyFrame leg compared with the oracle: 256 reached the kernel, whose keys
    // reserve dist > 255 for "nothing" -- wrong counts and an out-of-bounds store.)
    A.maxDist = Q.max_dist > 255 ? 255 : Q.max_dist < 0 ? 0 : Q.max_dist;
    pair.fill(A, P, dIn);
    A.lastKeys = (const ygzf_kp *) (dIn + (Q.last_keys ? oLastK : 0));   // not read in modes 1, 2: any valid address
    A.mpDesc = dIn + oMpD;
    A.world = dPX;     // unused in these modes
    A.mpValid = dTV;
    A.match12 = mode == 3 ? (int *) P.d_out(rM12) : nullptr;
    A.outlier = Q.is_bad ? dIn + oBad : nullptr;
    A.hasObs = Q.mp_has_obs ? dIn + oObs : nullptr;
    A.poses = (const float *) (dIn + oPose);
    A.mpProjX = dPX;
    A.mpProjY = dY;
    A.mpProjXR = dXR;
    A.mpViewCos = dVC;
    A.mpAngle = dVC;
    A.mpLevel = dLv;
    A.nnratio = Q.nnratio;
    fill_camera(A, cam, c);
    fill_view_scales(A, F);
    A.th = Q.th;
    A.bMono = 1;
    A.checkLevel = Q.check_level != 0;
    A.checkOri = Q.check_ori != 0;
    char label[16];
    snprintf(label, sizeof label, "mode %d", mode);
    if ((rc = run_match(c, A, 1, 0, label)) || (rc = P.download())) return rc;
    set_match_pairs(c, 0);
    return YGZF_OK;
}

// The node-wise searches' outputs (SearchByBoW, SearchForTriangulation): the match array, preset to -1 on the device, and a block of counters
// ([0] nmatches, [4 .. 34) the rotation histogram), zeroed.  add() before P.upload(), clear() after it, count() after P.download().
struct NodeSearchOut {
    int tail[64];
    size_t oMatch, oTail, matchBytes;
    void add(PackedTransfer &P, int *match, size_t n) {
        matchBytes = 4 * n;
        oMatch = P.add_out(match, matchBytes);
        oTail = P.add_out(tail, sizeof tail);
    }
    int *match(const PackedTransfer &P) const { return (int *) P.d_out(oMatch); }
    int *nmatches(const PackedTransfer &P) const { return (int *) P.d_out(oTail); }
    int *hist(const PackedTransfer &P) const { return nmatches(P) + 4; }
    int clear(ygzf_ctx *c, const PackedTransfer &P) const {
        HIPCHECK(c, hipMemsetAsync(match(P), 0xFF, matchBytes, c->stream));
        HIPCHECK(c, hipMemsetAsync(nmatches(P), 0, sizeof tail, c->stream));
        return YGZF_OK;
    }
    int count() const { return tail[0]; }
};

int ygzf_search_by_bow(ygzf_ctx *c, int n_nodes, const int *kf_off, const int *kf_idx, const int *f_off, const int *f_idx, int n_kf,
                       const uint8_t *kf_valid, const ygzf_kp *kf_keys, const uint8_t *kf_desc, int n_f, const ygzf_kp *f_keys, const uint8_t *f_desc,
                       float nnratio, int check_orientation, int *match, int *nmatches) {
    if (!c || !nmatches || (n_f > 0 && !match)) return fail(c, YGZF_ERR_INVALID, "null argument");
    *nmatches = 0;
    for (int i = 0; i < n_f; i++) match[i] = -1;   // vpMapPointMatches = vector<MapPoint*>(F.N, NULL)  (:158)
    if (n_nodes <= 0 || n_kf <= 0 || n_f <= 0) return YGZF_OK;
    if (!kf_off || !kf_idx || !f_off || !f_idx || !kf_valid || !kf_keys || !kf_desc || !f_keys || !f_desc) return fail(c, YGZF_ERR_INVALID, "null array");
    const int nk = kf_off[n_nodes], nfi = f_off[n_nodes];
    for (int k = 0; k < n_nodes; k++) {
        if (kf_off[k] > kf_off[k + 1] || f_off[k] > f_off[k + 1] || kf_off[k] < 0 || f_off[k] < 0) return fail(c, YGZF_ERR_INVALID, "node offsets not ascending");
        if (f_off[k + 1] - f_off[k] > 4096) return fail(c, YGZF_ERR_UNSUPPORTED, "more than 4096 frame features in one vocabulary node");
    }
    for (int i = 0; i < nk; i++) if (kf_idx[i] < 0 || kf_idx[i] >= n_kf) return fail(c, YGZF_ERR_INVALID, "KeyFrame feature index out of range");
    for (int i = 0; i < nfi; i++) if (f_idx[i] < 0 || f_idx[i] >= n_f) return fail(c, YGZF_ERR_INVALID, "Frame feature index out of range");
    HIPCHECK(c, hipSetDevice(c->device));
    // nine small host arrays in, two out: one packed copy each way (PackedTransfer; nine staged copies of their own until round 4)
    int rc;
    PackedTransfer P(c);
    const size_t iKO = P.add_in(kf_off, 4 * (size_t) (n_nodes + 1)), iKI = P.add_in(kf_idx, 4 * (size_t) nk), iFO = P.add_in(f_off, 4 * (size_t) (n_nodes + 1)),
                 iFI = P.add_in(f_idx, 4 * (size_t) nfi), iKV = P.add_in(kf_valid, (size_t) n_kf), iKK = P.add_in(kf_keys, sizeof(ygzf_kp) * (size_t) n_kf),
                 iKD = P.add_in(kf_desc, 32 * (size_t) n_kf), iFK = P.add_in(f_keys, sizeof(ygzf_kp) * (size_t) n_f), iFD = P.add_in(f_desc, 32 * (size_t) n_f);
    NodeSearchOut out;
    out.add(P, match, (size_t) n_f);
    uint8_t *d;
    if ((rc = P.upload(&d)) || (rc = ensure(c, c->dOwner, (size_t) n_f)) || (rc = out.clear(c, P))) return rc;
    {
        ProfScope ps(c, KK_BOWNODES);
        launch_bow(c->stream, n_nodes, (const int *) (d + iKO), (const int *) (d + iKI), (const int *) (d + iFO), (const int *) (d + iFI), d + iKV,
                   (const ygzf_kp *) (d + iKK), d + iKD, n_f, (const ygzf_kp *) (d + iFK), d + iFD, nnratio, check_orientation != 0, out.match(P),
                   (unsigned char *) c->dOwner.p, out.hist(P), out.nmatches(P));
    }
    HIPCHECK(c, hipGetLastError());
    if ((rc = P.download())) return rc;
    *nmatches = out.count();
    set_match_pairs(c, 0);
    return YGZF_OK;
}

// SearchByBoW(KF1, KF2) over n_cand KF2s (include/ygzf.h; match_kernels.hip: k_bow_kf_nodes).  Validation first; one packed copy in (KF1's
// arrays once, every candidate's arrays, the candidate table, the item prefix), one out.  Nothing in c->held is touched: only the packed staging
// area is written.
int ygzf_search_by_bow_kf(ygzf_ctx *c, int n1, const ygzf_kp *keys1, const uint8_t *desc1, const uint8_t *valid1, int n_cand,
                          const ygzf_bow_kf_candidate *cands, float nnratio, int check_orientation, int *match12, int *nmatches) {
    if (!c) return fail(c, YGZF_ERR_INVALID, "null argument");
    if (n1 < 0 || n_cand < 0) return fail(c, YGZF_ERR_INVALID, "negative count");
    if (n_cand > 0 && (!nmatches || !cands || (n1 > 0 && !match12))) return fail(c, YGZF_ERR_INVALID, "null argument");
    const size_t K = (size_t) n_cand, N1 = (size_t) n1;
    for (size_t k = 0; k < K; k++) nmatches[k] = 0;
    for (size_t i = 0; i < K * N1; i++) match12[i] = -1;   // vpMatches12 = vector<MapPoint*>(vpMapPoints1.size(), NULL)  (:491)
    if (n_cand == 0 || n1 == 0) return YGZF_OK;
    if (!keys1 || !desc1 || !valid1) return fail(c, YGZF_ERR_INVALID, "null array");
    std::vector<int> itemBase(K + 1, 0);
    for (int k = 0; k < n_cand; k++) {
        const ygzf_bow_kf_candidate &Q = cands[k];
        if (Q.n < 0 || Q.n_nodes < 0) return fail(c, YGZF_ERR_INVALID, "candidate %d: negative count", k);
        const bool empty = Q.n == 0 || Q.n_nodes == 0;
        itemBase[k + 1] = itemBase[k] + (empty ? 0 : Q.n_nodes);
        if (empty) continue;
        if (!Q.keys || !Q.desc || !Q.valid || !Q.off1 || !Q.idx1 || !Q.off2 || !Q.idx2) return fail(c, YGZF_ERR_INVALID, "candidate %d: null array", k);
        if (Q.off1[0] < 0 || Q.off2[0] < 0) return fail(c, YGZF_ERR_INVALID, "candidate %d: node offsets not ascending", k);
        for (int j = 0; j < Q.n_nodes; j++) {
            if (Q.off1[j] > Q.off1[j + 1] || Q.off2[j] > Q.off2[j + 1]) return fail(c, YGZF_ERR_INVALID, "candidate %d: node offsets not ascending", k);
            if (Q.off2[j + 1] - Q.off2[j] > 4096)
                return fail(c, YGZF_ERR_UNSUPPORTED, "candidate %d: more than 4096 features of the second KeyFrame in one vocabulary node", k);
        }
        for (int i = Q.off1[0]; i < Q.off1[Q.n_nodes]; i++)
            if (Q.idx1[i] < 0 || Q.idx1[i] >= n1) return fail(c, YGZF_ERR_INVALID, "candidate %d: feature index of the first KeyFrame out of range", k);
        for (int i = Q.off2[0]; i < Q.off2[Q.n_nodes]; i++)
            if (Q.idx2[i] < 0 || Q.idx2[i] >= Q.n) return fail(c, YGZF_ERR_INVALID, "candidate %d: feature index of the second KeyFrame out of range", k);
    }
    if (itemBase[K] == 0) return YGZF_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    int rc;
    PackedTransfer P(c);
    const size_t iK1 = P.add_in(keys1, sizeof(ygzf_kp) * N1), iD1 = P.add_in(desc1, 32 * N1), iV1 = P.add_in(valid1, N1);
    std::vector<BowKfCand> recs(K);
    memset(recs.data(), 0, sizeof(BowKfCand) * K);
    for (size_t k = 0; k < K; k++) {
        const ygzf_bow_kf_candidate &Q = cands[k];
        if (itemBase[k + 1] == itemBase[k]) continue;
        const size_t n = (size_t) Q.n, nn = (size_t) Q.n_nodes + 1;
        BowKfCand &R = recs[k];
        R.keys2 = (long long) P.add_in(Q.keys, sizeof(ygzf_kp) * n);
        R.desc2 = (long long) P.add_in(Q.desc, 32 * n);
        R.valid2 = (long long) P.add_in(Q.valid, n);
        R.off1 = (long long) P.add_in(Q.off1, 4 * nn);
        R.idx1 = (long long) P.add_in(Q.idx1, 4 * (size_t) Q.off1[Q.n_nodes]);
        R.off2 = (long long) P.add_in(Q.off2, 4 * nn);
        R.idx2 = (long long) P.add_in(Q.idx2, 4 * (size_t) Q.off2[Q.n_nodes]);
    }
    const size_t iR = P.add_in(recs.data(), sizeof(BowKfCand) * K), iB = P.add_in(itemBase.data(), 4 * (K + 1));
    std::vector<int> tail(K * kBowKfTail);
    const size_t oM = P.add_out(match12, 4 * K * N1), oT = P.add_out(tail.data(), 4 * tail.size()), oB = P.add_out(nullptr, K * N1);   // (binOf: scratch)
    uint8_t *d;
    if ((rc = P.upload(&d))) return rc;
    HIPCHECK(c, hipMemsetAsync(P.d_out(oM), 0xFF, 4 * K * N1, c->stream));
    HIPCHECK(c, hipMemsetAsync(P.d_out(oT), 0, 4 * tail.size(), c->stream));
    BowKfArgs A;
    A.nCand = n_cand; A.nItems = itemBase[K]; A.n1 = n1;
    A.base = d;
    A.cands = (const BowKfCand *) (d + iR);
    A.itemBase = (const int *) (d + iB);
    A.keys1 = (const ygzf_kp *) (d + iK1); A.desc1 = d + iD1; A.valid1 = d + iV1;
    A.nnratio = nnratio; A.checkOri = check_orientation != 0;
    A.match12 = (int *) P.d_out(oM);
    A.binOf = (unsigned char *) P.d_out(oB);
    A.tail = (int *) P.d_out(oT);
    {
        ProfScope ps(c, KK_BOWKF);
        launch_bow_kf(c->stream, A);
    }
    HIPCHECK(c, hipGetLastError());
    if ((rc = P.download())) return rc;
    for (size_t k = 0; k < K; k++) nmatches[k] = tail[k * kBowKfTail];
    return YGZF_OK;
}

int ygzf_search_for_triangulation(ygzf_ctx *c, int n_nodes, const int *off1, const int *idx1, const int *off2, const int *idx2,
                                  const ygzf_frame_view *kf1, const uint8_t *has_mp1, const ygzf_frame_view *kf2, const uint8_t *has_mp2,
                                  const float *level_sigma2_2, const float *F12, const float *Cw1, const float *R2w, const float *t2w,
                                  const ygzf_camera *cam2, int only_stereo, int check_orientation, int *match12, int *nmatches) {
    if (!c || !kf1 || !kf2 || !nmatches || (kf1->n > 0 && !match12)) return fail(c, YGZF_ERR_INVALID, "null argument");
    *nmatches = 0;
    const int n1 = kf1->n, n2 = kf2->n;
    for (int i = 0; i < n1; i++) match12[i] = -1;   // vMatches12 = vector<int>(pKF1->N, -1)  (:617)
    if (n_nodes <= 0 || n1 <= 0 || n2 <= 0) return YGZF_OK;
    if (!off1 || !idx1 || !off2 || !idx2 || !has_mp1 || !has_mp2 || !kf1->keys || !kf1->desc || !kf2->keys || !kf2->desc || !F12 || !Cw1 || !R2w ||
        !t2w || !cam2)
        return fail(c, YGZF_ERR_INVALID, "null array");
    const int L = kf2->scale_factors ? kf2->nlevels : c->tab.cfg.nlevels;
    if (L <= 0) return fail(c, YGZF_ERR_INVALID, "no scale levels");
    if (off1[0] != 0 || off2[0] != 0) return fail(c, YGZF_ERR_INVALID, "node offsets do not start at 0");
    for (int k = 0; k < n_nodes; k++) {
        if (off1[k] > off1[k + 1] || off2[k] > off2[k + 1]) return fail(c, YGZF_ERR_INVALID, "node offsets not ascending");
        if (off2[k + 1] - off2[k] > 65535) return fail(c, YGZF_ERR_UNSUPPORTED, "more than 65535 features of the second KeyFrame in one vocabulary node");
    }
    const int ne1 = off1[n_nodes], ne2 = off2[n_nodes];
    for (int i = 0; i < ne1; i++) if (idx1[i] < 0 || idx1[i] >= n1) return fail(c, YGZF_ERR_INVALID, "feature index of the first KeyFrame out of range");
    for (int i = 0; i < ne2; i++) if (idx2[i] < 0 || idx2[i] >= n2) return fail(c, YGZF_ERR_INVALID, "feature index of the second KeyFrame out of range");
    for (int i = 0; i < n2; i++)
        if (kf2->keys[i].octave < 0 || kf2->keys[i].octave >= L) return fail(c, YGZF_ERR_INVALID, "keypoint octave outside the scale tables");
    HIPCHECK(c, hipSetDevice(c->device));
    std::vector<float> sf(L), sg(L);
    for (int l = 0; l < L; l++) {
        sf[l] = kf2->scale_factors ? kf2->scale_factors[l] : c->tab.scale[l];
        sg[l] = level_sigma2_2 ? level_sigma2_2[l] : sf[l] * sf[l];   // mvLevelSigma2[i] = mvScaleFactor[i] * mvScaleFactor[i]  (src/ORBextractor.cc:422)
    }
    TriArgs A;
    {   // epipole in the second image (:601-608): C2 = R2w * Cw + t2w, coefficient order of the 3x3 product
        float C2[3];
        for (int r = 0; r < 3; r++) C2[r] = R2w[3 * r] * Cw1[0] + R2w[3 * r + 1] * Cw1[1] + R2w[3 * r + 2] * Cw1[2];
        for (int r = 0; r < 3; r++) C2[r] = C2[r] + t2w[r];
        const float invz = 1.0f / C2[2];
        A.ex = cam2->fx * C2[0] * invz + cam2->cx;
        A.ey = cam2->fy * C2[1] * invz + cam2->cy;
    }
    for (int i = 0; i < 9; i++) A.F[i] = F12[i];
    int rc;
    PackedTransfer P(c);
    const size_t N1 = (size_t) n1, N2 = (size_t) n2;
    const size_t iO1 = P.add_in(off1, 4 * (size_t) (n_nodes + 1)), iI1 = P.add_in(idx1, 4 * (size_t) ne1), iO2 = P.add_in(off2, 4 * (size_t) (n_nodes + 1)),
                 iI2 = P.add_in(idx2, 4 * (size_t) ne2), iK1 = P.add_in(kf1->keys, sizeof(ygzf_kp) * N1), iK2 = P.add_in(kf2->keys, sizeof(ygzf_kp) * N2),
                 iD1 = P.add_in(kf1->desc, 32 * N1), iD2 = P.add_in(kf2->desc, 32 * N2), iM1 = P.add_in(has_mp1, N1), iM2 = P.add_in(has_mp2, N2),
                 iU1 = P.add_in(kf1->u_right, kf1->u_right ? 4 * N1 : 0), iU2 = P.add_in(kf2->u_right, kf2->u_right ? 4 * N2 : 0),
                 iSf = P.add_in(sf.data(), 4 * (size_t) L), iSg = P.add_in(sg.data(), 4 * (size_t) L);
    NodeSearchOut out;
    out.add(P, match12, N1);
    uint8_t *d;
    if ((rc = P.upload(&d)) || (rc = ensure(c, c->dTriBinOf, N1 + 16)) || (rc = out.clear(c, P))) return rc;
    A.nEntries = ne1; A.nNodes = n_nodes; A.n1 = n1;
    A.off1 = (const int *) (d + iO1); A.idx1 = (const int *) (d + iI1); A.off2 = (const int *) (d + iO2); A.idx2 = (const int *) (d + iI2);
    A.keys1 = (const ygzf_kp *) (d + iK1); A.keys2 = (const ygzf_kp *) (d + iK2);
    A.desc1 = d + iD1; A.desc2 = d + iD2; A.hasMp1 = d + iM1; A.hasMp2 = d + iM2;
    A.uR1 = kf1->u_right ? (const float *) (d + iU1) : nullptr;
    A.uR2 = kf2->u_right ? (const float *) (d + iU2) : nullptr;
    A.sf2 = (const float *) (d + iSf); A.sigma2 = (const float *) (d + iSg);
    A.onlyStereo = only_stereo != 0; A.checkOri = check_orientation != 0;
    A.match12 = out.match(P);
    A.binOf = (unsigned char *) c->dTriBinOf.p;
    A.nmatches = out.nmatches(P);
    A.hist = out.hist(P);
    {
        ProfScope ps(c, KK_TRI);
        launch_triangulation(c->stream, A);
    }
    HIPCHECK(c, hipGetLastError());
    if ((rc = P.download())) return rc;
    *nmatches = out.count();
    set_match_pairs(c, 0);
    return YGZF_OK;
}

}  // extern "C" (the next two are the library's own, shared with ygzf_api_kfstore.hip: ygzf_ctx.h)

// One keyframe of the Fuse / loop-closing searches: the argument checks (needSigma: mvInvLevelSigma2 is read, i.e. the first Fuse) ...
int kf_args_check(ygzf_ctx *c, const ygzf_frame_view &view, const ygzf_camera &cam, const float *inv_level_sigma2, int k, bool needSigma) {
    const int n = view.n;
    if (n < 0) return fail(c, YGZF_ERR_INVALID, "keyframe %d: negative key count", k);
    if (n > 0 && (!view.keys || !view.desc)) return fail(c, YGZF_ERR_INVALID, "keyframe %d: null key array", k);
    if (needSigma && !inv_level_sigma2) return fail(c, YGZF_ERR_INVALID, "keyframe %d: null mvInvLevelSigma2", k);
    const int L = view.scale_factors ? view.nlevels : c->tab.cfg.nlevels;
    if (L < 1 || L > kMaxLevels) return fail(c, YGZF_ERR_INVALID, "keyframe %d: nlevels out of range", k);
    if (!(cam.max_x > cam.min_x) || !(cam.max_y > cam.min_y)) return fail(c, YGZF_ERR_INVALID, "keyframe %d: empty image bounds", k);
    for (int i = 0; i < n; i++)
        if (view.keys[i].octave < 0 || view.keys[i].octave >= L)
            return fail(c, YGZF_ERR_INVALID, "keyframe %d: keypoint octave outside the scale tables", k);
    if (n > kGridMaxKeys) return fail(c, YGZF_ERR_UNSUPPORTED, "keyframe %d: more than %d keypoints in one grid", k, kGridMaxKeys);
    return YGZF_OK;
}
// ... and its device record: what does not depend on the pose or on where the arrays lie (a resident keyframe keeps this part) ...
void kf_record_static(ygzf_ctx *c, const ygzf_frame_view &view, const ygzf_camera &cam, const float *inv_level_sigma2, float log_scale_factor, FuseKf &F) {
    memset(&F, 0, sizeof F);
    F.n = view.n;
    F.nLevels = view.scale_factors ? view.nlevels : c->tab.cfg.nlevels;
    F.fx = cam.fx; F.fy = cam.fy; F.cx = cam.cx; F.cy = cam.cy; F.mbf = cam.mbf;
    F.minX = cam.min_x; F.minY = cam.min_y; F.maxX = cam.max_x; F.maxY = cam.max_y;
    grid_inverses(cam, F.gridInvW, F.gridInvH);
    predict_scale_steps(log_scale_factor, F.nLevels, F.levelStep);
    for (int l = 0; l < kMaxLevels; l++) {
        F.scale[l] = l < F.nLevels ? (view.scale_factors ? view.scale_factors[l] : c->tab.scale[l]) : 1.f;
        F.invSigma2[l] = l < F.nLevels && inv_level_sigma2 ? inv_level_sigma2[l] : 1.f;
    }
}
extern "C" {
static int fuse_kf_check(ygzf_ctx *c, const ygzf_fuse_kf &K, int k, bool needSigma) { return kf_args_check(c, K.view, K.cam, K.inv_level_sigma2, k, needSigma); }
// ... with the pose; the key arrays join the packed upload
static void fuse_kf_fill(ygzf_ctx *c, PackedTransfer &P, const ygzf_fuse_kf &K, FuseKf &F) {
    kf_record_static(c, K.view, K.cam, K.inv_level_sigma2, K.log_scale_factor, F);
    const size_t n = (size_t) K.view.n;
    F.keys = (long long) P.add_in(K.view.keys, sizeof(ygzf_kp) * n);
    F.desc = (long long) P.add_in(K.view.desc, 32 * n);
    F.uRight = K.view.u_right ? (long long) P.add_in(K.view.u_right, 4 * n) : -1;
    memcpy(F.Rcw, K.Rcw, 36);
    memcpy(F.tcw, K.tcw, 12);
    memcpy(F.Ow, K.Ow, 12);
}

// ---- the projection searches of one snapshot (include/ygzf.h; match_kernels.hip: k_proj_search) -------------------------------------------
// Validation first; one packed copy in (every keyframe's keys / descriptors / mvuRight, the point arrays, the skip masks, the row table), one
// out.  Nothing in c->held is touched: only the packed staging area is written.
static int proj_points_check(ygzf_ctx *c, const ygzf_fuse_points *pts, bool needNormal) {
    if (!pts->world || (needNormal && !pts->normal) || !pts->max_dist_inv || !pts->min_dist_inv || !pts->mf_max_distance || !pts->desc)
        return fail(c, YGZF_ERR_INVALID, "null point array");
    return YGZF_OK;
}
static void proj_row_points(PackedTransfer &P, ProjRow &R, const ygzf_fuse_points *pts, int n, bool withNormal, const uint8_t *skip) {
    const size_t N = (size_t) n;
    R.world = (long long) P.add_in(pts->world, 12 * N);
    R.normal = withNormal ? (long long) P.add_in(pts->normal, 12 * N) : -1;
    R.maxDistInv = (long long) P.add_in(pts->max_dist_inv, 4 * N);
    R.minDistInv = (long long) P.add_in(pts->min_dist_inv, 4 * N);
    R.mfMaxDistance = (long long) P.add_in(pts->mf_max_distance, 4 * N);
    R.mpDesc = (long long) P.add_in(pts->desc, 32 * N);
    R.skip = skip ? (long long) P.add_in(skip, N) : -1;
    R.keyMatched = -1;
    R.nPoints = n;
}
static int proj_run(ygzf_ctx *c, PackedTransfer &P, std::vector<ProjRow> &rows, int mode, int slot, int maxPoints, int maxKeys, float th, int nBest,
                    int maxHamming, size_t oI, size_t oD, const uint8_t *kfBase = nullptr) {
    int rc;
    const size_t iR = P.add_in(rows.data(), sizeof(ProjRow) * rows.size());
    uint8_t *d;
    if ((rc = P.upload(&d))) return rc;
    ProjArgs A;
    A.mode = mode;
    A.nRows = (int) rows.size(); A.maxPoints = maxPoints;
    A.slice = 64;   // points per workgroup (four per wave): a forward Fuse of 20 keyframes x 1 500 points and a reverse one of 1 x 30 000 both give ~500 workgroups
    A.base = d;
    A.kfBase = kfBase;
    A.rows = (const ProjRow *) (d + iR);
    A.th = th;
    A.nBest = nBest; A.maxHamming = maxHamming;
    A.bestIdx = (int *) P.d_out(oI);
    A.bestDist = (int *) P.d_out(oD);
    {
        ProfScope ps(c, slot);
        HIPCHECK(c, launch_proj_search(c->stream, A, maxKeys));
    }
    HIPCHECK(c, hipGetLastError());
    return P.download();
}

// K keyframes x one point list, a row per keyframe: ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th), src/ORBmatcher.cc:764-868
// (PM_FUSE; reads mvInvLevelSigma2) and LoopClosing's Fuse(pKF, Scw, ...), :888-1004 (PM_FUSE_SCW)
static int fuse_rows(ygzf_ctx *c, int mode, bool needSigma, int slot, int n_kf, const ygzf_fuse_kf *kfs, int n_points, const ygzf_fuse_points *pts,
                     const uint8_t *skip, float th, int *best_idx, int *best_dist) {
    if (!c) return fail(c, YGZF_ERR_INVALID, "null argument");
    if (n_kf < 0 || n_points < 0) return fail(c, YGZF_ERR_INVALID, "negative count");
    if (n_kf == 0 || n_points == 0) return YGZF_OK;
    if (!kfs || !pts || !best_idx || !best_dist) return fail(c, YGZF_ERR_INVALID, "null argument");
    int rc, maxKeys = 0;
    if ((rc = proj_points_check(c, pts, true))) return rc;
    for (int k = 0; k < n_kf; k++) {
        if ((rc = fuse_kf_check(c, kfs[k], k, needSigma))) return rc;
        maxKeys = std::max(maxKeys, kfs[k].view.n);
    }
    HIPCHECK(c, hipSetDevice(c->device));
    PackedTransfer P(c);
    std::vector<ProjRow> rows((size_t) n_kf);
    memset(rows.data(), 0, sizeof(ProjRow) * rows.size());
    const size_t N = (size_t) n_points;
    proj_row_points(P, rows[0], pts, n_points, true, nullptr);   // one copy of the point arrays, shared by every row
    const long long iS = skip ? (long long) P.add_in(skip, (size_t) n_kf * N) : -1;
    for (int k = 0; k < n_kf; k++) {
        if (k) rows[k] = rows[0];
        fuse_kf_fill(c, P, kfs[k], rows[k].kf);
        rows[k].skip = skip ? iS + (long long) ((size_t) k * N) : -1;
        rows[k].out = (long long) ((size_t) k * N);
    }
    const size_t oI = P.add_out(best_idx, 4 * N * n_kf), oD = P.add_out(best_dist, 4 * N * n_kf);
    return proj_run(c, P, rows, mode, slot, n_points, maxKeys, th, 1, 255, oI, oD);
}

int ygzf_fuse_candidates(ygzf_ctx *c, int n_kf, const ygzf_fuse_kf *kfs, int n_points, const ygzf_fuse_points *pts, const uint8_t *skip, float th,
                         int *best_idx, int *best_dist) {
    return fuse_rows(c, PM_FUSE, true, KK_FUSE, n_kf, kfs, n_points, pts, skip, th, best_idx, best_dist);
}

int ygzf_fuse_sim3_candidates(ygzf_ctx *c, int n_kf, const ygzf_fuse_kf *kfs, int n_points, const ygzf_fuse_points *pts, const uint8_t *skip, float th,
                              int *best_idx, int *best_dist) {
    return fuse_rows(c, PM_FUSE_SCW, false, KK_PROJ, n_kf, kfs, n_points, pts, skip, th, best_idx, best_dist);
}

// The two Fuse members over resident keyframes (ygzf_api_kfstore.hip): fuse_rows with every row's keyframe taken from the store.  Only the
// point arrays, the skip mask and the row table cross the link; a row's record is the slot's own, moved to where the row lies in the arena, with
// the call's pose.
static int fuse_rows_resident(ygzf_ctx *c, int mode, bool needSigma, int slot, int n_kf, const ygzf_kf_ref *refs, int n_points, const ygzf_fuse_points *pts,
                              const uint8_t *skip, float th, int *best_idx, int *best_dist) {
    if (!c) return fail(c, YGZF_ERR_INVALID, "null argument");
    if (n_kf < 0 || n_points < 0) return fail(c, YGZF_ERR_INVALID, "negative count");
    if (n_kf == 0 || n_points == 0) return YGZF_OK;
    if (!best_idx || !best_dist) return fail(c, YGZF_ERR_INVALID, "null argument");
    const size_t N = (size_t) n_points, E = N * (size_t) n_kf;
    for (size_t i = 0; i < E; i++) { best_idx[i] = -1; best_dist[i] = 256; }
    if (!refs || !pts) return fail(c, YGZF_ERR_INVALID, "null argument");
    int rc;
    if ((rc = proj_points_check(c, pts, true))) return rc;
    const ygzf_ctx::KfStore &S = c->kfs;
    for (int k = 0; k < n_kf; k++) {
        const auto it = S.slotOf.find(refs[k].key);
        if (it == S.slotOf.end()) return fail(c, YGZF_ERR_INVALID, "keyframe %d: key %llu is not resident", k, (unsigned long long) refs[k].key);
        if (needSigma && !S.slots[it->second].hasSigma) return fail(c, YGZF_ERR_INVALID, "keyframe %d: put without mvInvLevelSigma2", k);
    }
    HIPCHECK(c, hipSetDevice(c->device));
    PackedTransfer P(c);
    std::vector<ProjRow> rows((size_t) n_kf);
    memset(rows.data(), 0, sizeof(ProjRow) * rows.size());
    proj_row_points(P, rows[0], pts, n_points, true, nullptr);   // one copy of the point arrays, shared by every row
    const long long iS = skip ? (long long) P.add_in(skip, (size_t) n_kf * N) : -1;
    for (int k = 0; k < n_kf; k++) {
        if (k) rows[k] = rows[0];
        const ygzf_ctx::KfStore::Slot &L = S.slots[S.slotOf.at(refs[k].key)];
        FuseKf &F = rows[k].kf;
        F = L.kf;
        F.keys += L.off;
        F.desc += L.off;
        if (F.uRight >= 0) F.uRight += L.off;
        memcpy(F.Rcw, refs[k].Rcw, 36);
        memcpy(F.tcw, refs[k].tcw, 12);
        memcpy(F.Ow, refs[k].Ow, 12);
        rows[k].cellStart = L.off + L.cellStart;
        rows[k].list = L.off + L.list;
        rows[k].skip = skip ? iS + (long long) ((size_t) k * N) : -1;
        rows[k].out = (long long) ((size_t) k * N);
    }
    const size_t oI = P.add_out(best_idx, 4 * E), oD = P.add_out(best_dist, 4 * E);
    return proj_run(c, P, rows, mode, slot, n_points, 0, th, 1, 255, oI, oD, (const uint8_t *) S.dArena.p);
}

int ygzf_fuse_candidates_resident(ygzf_ctx *c, int n_kf, const ygzf_kf_ref *refs, int n_points, const ygzf_fuse_points *pts, const uint8_t *skip, float th,
                                  int *best_idx, int *best_dist) {
    return fuse_rows_resident(c, PM_FUSE, true, KK_FUSE, n_kf, refs, n_points, pts, skip, th, best_idx, best_dist);
}

int ygzf_fuse_sim3_candidates_resident(ygzf_ctx *c, int n_kf, const ygzf_kf_ref *refs, int n_points, const ygzf_fuse_points *pts, const uint8_t *skip,
                                       float th, int *best_idx, int *best_dist) {
    return fuse_rows_resident(c, PM_FUSE_SCW, false, KK_PROJ, n_kf, refs, n_points, pts, skip, th, best_idx, best_dist);
}

int ygzf_search_by_projection_sim3(ygzf_ctx *c, const ygzf_fuse_kf *kf, int n_points, const ygzf_fuse_points *pts, const uint8_t *skip,
                                   const uint8_t *key_matched, float th, int n_best, int max_dist, int *cand_idx, int *cand_dist) {
    if (!c) return fail(c, YGZF_ERR_INVALID, "null argument");
    if (n_points < 0) return fail(c, YGZF_ERR_INVALID, "negative count");
    if (n_best < 1 || n_best > 8) return fail(c, YGZF_ERR_INVALID, "n_best %d outside 1..8", n_best);
    if (max_dist < 0 || max_dist > 255) return fail(c, YGZF_ERR_INVALID, "max_dist %d outside 0..255", max_dist);
    if (n_points == 0) return YGZF_OK;
    if (!kf || !pts || !cand_idx || !cand_dist) return fail(c, YGZF_ERR_INVALID, "null argument");
    int rc;
    if ((rc = proj_points_check(c, pts, true)) || (rc = fuse_kf_check(c, *kf, 0, false))) return rc;
    HIPCHECK(c, hipSetDevice(c->device));
    PackedTransfer P(c);
    std::vector<ProjRow> rows(1);
    memset(rows.data(), 0, sizeof(ProjRow));
    proj_row_points(P, rows[0], pts, n_points, true, skip);
    fuse_kf_fill(c, P, *kf, rows[0].kf);
    if (key_matched && kf->view.n > 0) rows[0].keyMatched = (long long) P.add_in(key_matched, (size_t) kf->view.n);
    const size_t E = (size_t) n_points * (size_t) n_best;
    const size_t oI = P.add_out(cand_idx, 4 * E), oD = P.add_out(cand_dist, 4 * E);
    return proj_run(c, P, rows, PM_PROJ_SCW, KK_PROJ, n_points, kf->view.n, th, n_best, max_dist, oI, oD);
}

int ygzf_search_by_sim3(ygzf_ctx *c, const ygzf_fuse_kf *kf1, const ygzf_fuse_kf *kf2, const ygzf_fuse_points *pts1, const ygzf_fuse_points *pts2,
                        const uint8_t *skip1, const uint8_t *skip2, const ygzf_sim3_transforms *T, float th, int th_dist, int *match1, int *match2,
                        int *match12, int *nfound) {
    if (!c || !kf1 || !kf2 || !T || !nfound) return fail(c, YGZF_ERR_INVALID, "null argument");
    *nfound = 0;
    const int n1 = kf1->view.n, n2 = kf2->view.n;
    int rc;
    if ((rc = fuse_kf_check(c, *kf1, 1, false)) || (rc = fuse_kf_check(c, *kf2, 2, false))) return rc;
    if ((n1 > 0 && (!pts1 || !match1 || !match12)) || (n2 > 0 && (!pts2 || !match2))) return fail(c, YGZF_ERR_INVALID, "null argument");
    if ((n1 > 0 && (rc = proj_points_check(c, pts1, false))) || (n2 > 0 && (rc = proj_points_check(c, pts2, false)))) return rc;
    for (int i = 0; i < n1; i++) match1[i] = match12[i] = -1;
    for (int i = 0; i < n2; i++) match2[i] = -1;
    if (n1 == 0 || n2 == 0) return YGZF_OK;   // either direction finds no key, or has no point, and nothing can agree
    HIPCHECK(c, hipSetDevice(c->device));
    PackedTransfer P(c);
    std::vector<ProjRow> rows(2);
    memset(rows.data(), 0, sizeof(ProjRow) * 2);
    // row 0: KF1's points into KF2 (R1w, t1w then sR21, t21); row 1: KF2's points into KF1 (R2w, t2w then sR12, t12)
    proj_row_points(P, rows[0], pts1, n1, false, skip1);
    fuse_kf_fill(c, P, *kf2, rows[0].kf);
    memcpy(rows[0].kf.Rcw, T->R1w, 36); memcpy(rows[0].kf.tcw, T->t1w, 12);
    memcpy(rows[0].R2, T->sR21, 36); memcpy(rows[0].t2, T->t21, 12);
    rows[0].out = 0;
    proj_row_points(P, rows[1], pts2, n2, false, skip2);
    fuse_kf_fill(c, P, *kf1, rows[1].kf);
    memcpy(rows[1].kf.Rcw, T->R2w, 36); memcpy(rows[1].kf.tcw, T->t2w, 12);
    memcpy(rows[1].R2, T->sR12, 36); memcpy(rows[1].t2, T->t12, 12);
    rows[1].out = n1;
    std::vector<int> bi((size_t) n1 + n2), bd((size_t) n1 + n2);
    const size_t oI = P.add_out(bi.data(), 4 * bi.size()), oD = P.add_out(bd.data(), 4 * bd.size());
    if ((rc = proj_run(c, P, rows, PM_SIM3, KK_PROJ, std::max(n1, n2), std::max(n1, n2), th, 1, 255, oI, oD))) return rc;
    for (int i = 0; i < n1; i++) match1[i] = bd[i] <= th_dist ? bi[i] : -1;                 // :1119-1121
    for (int i = 0; i < n2; i++) match2[i] = bd[n1 + i] <= th_dist ? bi[n1 + i] : -1;       // :1195-1197
    int found = 0;
    for (int i1 = 0; i1 < n1; i1++) {                                                       // :1200-1213
        const int idx2 = match1[i1];
        if (idx2 >= 0 && match2[idx2] == i1) { match12[i1] = idx2; found++; }
    }
    *nfound = found;
    return YGZF_OK;
}

int ygzf_search_for_initialization(ygzf_ctx *c, const ygzf_frame_view *F1, const ygzf_frame_view *F2, const ygzf_camera *cam, float *prev_matched_xy,
                                   int window_size, float nnratio, int check_orientation, int *matches12, int *nmatches) {
    if (!c || !F1 || !F2 || !cam || !nmatches || !matches12 || !prev_matched_xy) return fail(c, YGZF_ERR_INVALID, "null argument");
    *nmatches = 0;
    for (int i = 0; i < F1->n; i++) matches12[i] = -1;   // vnMatches12 = vector<int>(F1.N, -1)  (:379)
    if (F1->n <= 0 || F2->n <= 0) return YGZF_OK;
    std::vector<float> px(F1->n), py(F1->n);
    for (int i = 0; i < F1->n; i++) { px[i] = prev_matched_xy[2 * i]; py[i] = prev_matched_xy[2 * i + 1]; }
    std::vector<uint8_t> owner(F2->n, 0);
    std::vector<int> match21(F2->n, -1);
    ProjectedQuery Q = {};
    Q.mode = 3; Q.n_mp = F1->n;
    Q.proj_x = px.data(); Q.proj_y = py.data();
    Q.mp_desc = F1->desc;
    Q.th = (float) window_size; Q.nnratio = nnratio; Q.max_dist = 50; Q.check_ori = check_orientation;
    Q.owner = owner.data(); Q.match = match21.data(); Q.nmatches = nmatches;
    Q.last_keys = F1->keys; Q.match12 = matches12;
    int rc = projected_match(c, F2, cam, Q);
    if (rc) return rc;
    for (int i = 0; i < F1->n; i++)      // :470-474 update prev matched
        if (matches12[i] >= 0) {
            prev_matched_xy[2 * i] = F2->keys[matches12[i]].x;
            prev_matched_xy[2 * i + 1] = F2->keys[matches12[i]].y;
        }
    return YGZF_OK;
}

int ygzf_search_by_projection_mappoints(ygzf_ctx *c, const ygzf_frame_view *F, const ygzf_camera *cam, int n_mp, const uint8_t *track_in_view,
                                        const uint8_t *is_bad, const uint8_t *mp_has_obs, const float *proj_x, const float *proj_y,
                                        const float *proj_xr, const float *view_cos, const int *scale_level, const uint8_t *mp_desc, float th,
                                        int check_level, float nnratio, uint8_t *owner, int *match, int *nmatches) {
    ProjectedQuery Q = {};
    Q.mode = 1; Q.n_mp = n_mp;
    Q.track_in_view = track_in_view; Q.is_bad = is_bad; Q.mp_has_obs = mp_has_obs;
    Q.proj_x = proj_x; Q.proj_y = proj_y; Q.proj_xr = proj_xr; Q.view_cos = view_cos; Q.scale_level = scale_level;
    Q.mp_desc = mp_desc;
    Q.th = th; Q.check_level = check_level; Q.nnratio = nnratio; Q.max_dist = 100;
    Q.owner = owner; Q.match = match; Q.nmatches = nmatches;
    return projected_match(c, F, cam, Q);
}

int ygzf_predict_scale_steps(float log_scale_factor, int nlevels, float *steps) {
    if (!steps || nlevels < 1 || nlevels > kMaxLevels) return YGZF_ERR_INVALID;
    float st[kMaxLevels];
    predict_scale_steps(log_scale_factor, nlevels, st);
    for (int k = 0; k < nlevels; k++) steps[k] = k == 0 ? 0.f : st[k];
    return YGZF_OK;
}

int ygzf_is_in_frustum_batch(ygzf_ctx *c, const ygzf_camera *cam, int nlevels, int n, const ygzf_frustum_in *in, uint8_t *in_view, float *proj_x,
                             float *proj_y, float *proj_xr, int *level, float *view_cos) {
    if (!c || !cam || !in || !in_view || !proj_x || !proj_y || !proj_xr || !level || !view_cos) return fail(c, YGZF_ERR_INVALID, "null argument");
    if (n < 0) return fail(c, YGZF_ERR_INVALID, "negative count");
    if (n == 0) return YGZF_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    int rc;
    PackedTransfer P(c);
    FrustumOffsets FO;
    if ((rc = frustum_add_inputs(c, P, FO, in, n, nlevels))) return rc;
    const size_t N = (size_t) n;
    const size_t rPX = P.add_out(proj_x, 4 * N), rPY = P.add_out(proj_y, 4 * N), rPXR = P.add_out(proj_xr, 4 * N), rVC = P.add_out(view_cos, 4 * N),
                 rLv = P.add_out(level, 4 * N), rIV = P.add_out(in_view, N);
    uint8_t *dIn;
    if ((rc = P.upload(&dIn))) return rc;
    FrustumArgs A;
    frustum_fill_args(A, dIn, FO, in, cam, n, nlevels);
    A.inView = P.d_out(rIV);
    A.projX = (float *) P.d_out(rPX); A.projY = (float *) P.d_out(rPY); A.projXR = (float *) P.d_out(rPXR); A.viewCos = (float *) P.d_out(rVC);
    A.level = (int *) P.d_out(rLv);
    HIPCHECK(c, hipMemsetAsync(P.d_out(0), 0, P.outBytes, c->stream));   // rejected points read as zeros
    {
        ProfScope ps(c, KK_FRUSTUM);
        launch_frustum(c->stream, A);
    }
    HIPCHECK(c, hipGetLastError());
    return P.download();
}

int ygzf_search_local_points(ygzf_ctx *c, const ygzf_frame_view *F, const ygzf_camera *cam, int n_mp, const ygzf_frustum_in *in,
                             const uint8_t *mp_has_obs, const uint8_t *mp_desc, float th, int check_level, float nnratio, uint8_t *owner, int *match,
                             int *nmatches, uint8_t *in_view, float *proj_x, float *proj_y, float *proj_xr, int *level, float *view_cos) {
    if (!in) return fail(c, YGZF_ERR_INVALID, "null argument");
    FrustumHost fr = {in, in_view, proj_x, proj_y, proj_xr, view_cos, level};
    ProjectedQuery Q = {};
    Q.mode = 1; Q.n_mp = n_mp;
    Q.mp_has_obs = mp_has_obs; Q.mp_desc = mp_desc;
    Q.th = th; Q.check_level = check_level; Q.nnratio = nnratio; Q.max_dist = 100;
    Q.owner = owner; Q.match = match; Q.nmatches = nmatches;
    Q.fr = &fr;
    return projected_match(c, F, cam, Q);
}

int ygzf_features_in_area(ygzf_ctx *c, const ygzf_camera *cam, int n_keys, const ygzf_kp *keys, int n_queries, const float *xyr, const int *levels,
                          int cap, int *out_idx, int *out_n) {
    if (!c || !cam || (n_keys > 0 && !keys) || (n_queries > 0 && (!xyr || !out_n)) || (n_queries > 0 && cap > 0 && !out_idx))
        return fail(c, YGZF_ERR_INVALID, "null argument");
    if (n_keys < 0 || n_queries < 0 || cap < 0) return fail(c, YGZF_ERR_INVALID, "negative count");
    if (!(cam->max_x > cam->min_x) || !(cam->max_y > cam->min_y)) return fail(c, YGZF_ERR_INVALID, "empty image bounds");
    if (n_queries == 0) return YGZF_OK;
    if (n_keys > kGridMaxKeys) return fail(c, YGZF_ERR_UNSUPPORTED, "more than %d keypoints in one grid", kGridMaxKeys);
    HIPCHECK(c, hipSetDevice(c->device));
    int rc;
    const size_t qBytes = (size_t) n_queries * 12, lBytes = levels ? (size_t) n_queries * 8 : 0;
    const size_t oBytes = (size_t) n_queries * (size_t) cap * 4, nBytes = (size_t) n_queries * 4;
    const size_t nPad = (nBytes + 15) & ~(size_t) 15;
    const size_t kBytes = (size_t) n_keys * sizeof(ygzf_kp);
    const bool packed = kBytes + qBytes + lBytes + nBytes + oBytes <= kPackedMax;   // one packed copy each way; beyond that, staged copies
    FiaArgs A;
    A.n = n_keys;
    A.minX = cam->min_x; A.minY = cam->min_y;
    grid_inverses(*cam, A.gridInvW, A.gridInvH);
    A.nq = n_queries;
    A.cap = cap;
    PackedTransfer P(c);
    if (packed) {
        const size_t iK = P.add_in(keys, kBytes), iQ = P.add_in(xyr, qBytes), iL = P.add_in(levels, lBytes);
        const size_t oN = P.add_out(out_n, nBytes), oI = P.add_out(out_idx, oBytes);
        uint8_t *d;
        if ((rc = P.upload(&d))) return rc;
        A.keys = (const ygzf_kp *) (d + iK);
        A.xyr = (const float *) (d + iQ);
        A.levels = levels ? (const int *) (d + iL) : nullptr;
        A.outN = (int *) P.d_out(oN);
        A.outIdx = (int *) P.d_out(oI);
    } else {
        if ((rc = ensure_scratch(c, c->tmp.a, kBytes + 64)) || (rc = ensure_scratch(c, c->tmp.b, qBytes + lBytes + 64)) || (rc = ensure_scratch(c, c->tmp.c, nPad + oBytes + 64)))
            return rc;
        if (n_keys > 0) HIPCHECK(c, hipMemcpyAsync(c->tmp.a.p, keys, kBytes, hipMemcpyHostToDevice, c->stream));
        HIPCHECK(c, hipMemcpyAsync(c->tmp.b.p, xyr, qBytes, hipMemcpyHostToDevice, c->stream));
        if (levels) HIPCHECK(c, hipMemcpyAsync((uint8_t *) c->tmp.b.p + qBytes, levels, lBytes, hipMemcpyHostToDevice, c->stream));
        A.keys = (const ygzf_kp *) c->tmp.a.p;
        A.xyr = (const float *) c->tmp.b.p;
        A.levels = levels ? (const int *) ((uint8_t *) c->tmp.b.p + qBytes) : nullptr;
        A.outN = (int *) c->tmp.c.p;
        A.outIdx = (int *) ((uint8_t *) c->tmp.c.p + nPad);
    }
    {
        ProfScope ps(c, KK_GRID);
        HIPCHECK(c, launch_features_in_area(c->stream, A));
    }
    HIPCHECK(c, hipGetLastError());
    if (packed) return P.download();
    HIPCHECK(c, hipMemcpyAsync(out_n, A.outN, nBytes, hipMemcpyDeviceToHost, c->stream));
    if (oBytes) HIPCHECK(c, hipMemcpyAsync(out_idx, A.outIdx, oBytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return YGZF_OK;
}

int ygzf_distinctive_descriptors_batch(ygzf_ctx *c, int n_points, const int *obs_off, const uint8_t *desc, int *best_idx) {
    if (!c || (n_points > 0 && (!obs_off || !best_idx))) return fail(c, YGZF_ERR_INVALID, "null argument");
    if (n_points <= 0) return YGZF_OK;
    const int total = obs_off[n_points];
    std::vector<int> large;          // points beyond the register-resident form (> 256 observations): the histogram kernel's
    for (int p = 0; p < n_points; p++) {
        const int n = obs_off[p + 1] - obs_off[p];
        if (n < 0 || obs_off[p] < 0) return fail(c, YGZF_ERR_INVALID, "observation offsets not ascending");
        if (n > 256) large.push_back(p);
    }
    if (total > 0 && !desc) return fail(c, YGZF_ERR_INVALID, "null descriptors");
    HIPCHECK(c, hipSetDevice(c->device));
    int rc;
    const size_t offBytes = (4 * (size_t) (n_points + 1) + 15) & ~(size_t) 15;
    if ((rc = ensure_scratch(c, c->tmp.a, offBytes + 4 * large.size() + 16)) || (rc = ensure_scratch(c, c->tmp.b, 4 * (size_t) n_points)) ||
        (rc = ensure_scratch(c, c->tmp.c, 32 * (size_t) (total + 1))))
        return rc;
    HIPCHECK(c, hipMemcpyAsync(c->tmp.a.p, obs_off, 4 * (size_t) (n_points + 1), hipMemcpyHostToDevice, c->stream));
    if (!large.empty()) HIPCHECK(c, hipMemcpyAsync((uint8_t *) c->tmp.a.p + offBytes, large.data(), 4 * large.size(), hipMemcpyHostToDevice, c->stream));
    if (total > 0) HIPCHECK(c, hipMemcpyAsync(c->tmp.c.p, desc, 32 * (size_t) total, hipMemcpyHostToDevice, c->stream));
    {
        ProfScope ps(c, KK_DISTINCTIVE);
        launch_distinctive(c->stream, n_points, (const int *) c->tmp.a.p, (const uint8_t *) c->tmp.c.p, (int *) c->tmp.b.p, (int) large.size(),
                           (const int *) ((uint8_t *) c->tmp.a.p + offBytes));
    }
    HIPCHECK(c, hipGetLastError());
    HIPCHECK(c, hipMemcpyAsync(best_idx, c->tmp.b.p, 4 * (size_t) n_points, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return YGZF_OK;
}

// ---- Frame::ComputeBoW: vocabulary on the device + tree descent ------------------------------------------------------------------------
int ygzf_vocabulary_set(ygzf_ctx *c, int n_nodes, int depth_levels, const int *parent, const uint8_t *desc) {
    if (!c || !parent || !desc) return fail(c, YGZF_ERR_INVALID, "null argument");
    if (n_nodes < 1 || depth_levels < 0) return fail(c, YGZF_ERR_INVALID, "bad vocabulary size");
    HIPCHECK(c, hipSetDevice(c->device));
    // children lists in ascending node id (= the loaders' push_back order), as CSR
    std::vector<int> off((size_t) n_nodes + 1, 0), idx((size_t) std::max(n_nodes - 1, 1));
    for (int i = 1; i < n_nodes; i++) {
        if (parent[i] < 0 || parent[i] >= n_nodes || parent[i] == i) return fail(c, YGZF_ERR_INVALID, "node %d: parent %d out of range", i, parent[i]);
        off[(size_t) parent[i] + 1]++;
    }
    for (int i = 0; i < n_nodes; i++) off[(size_t) i + 1] += off[i];
    {
        std::vector<int> fill(off.begin(), off.end() - 1);
        for (int i = 1; i < n_nodes; i++) idx[(size_t) fill[parent[i]]++] = i;
    }
    int rc;
    if ((rc = ensure(c, c->voc.childOff, off.size() * sizeof(int))) || (rc = ensure(c, c->voc.childIdx, idx.size() * sizeof(int))) ||
        (rc = ensure(c, c->voc.nodeDesc, (size_t) n_nodes * 32)))
        return rc;
    c->vocNodes = 0;
    HIPCHECK(c, hipMemcpyAsync(c->voc.childOff.p, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(c, hipMemcpyAsync(c->voc.childIdx.p, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(c, hipMemcpyAsync(c->voc.nodeDesc.p, desc, (size_t) n_nodes * 32, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    c->vocNodes = n_nodes;
    c->vocLevels = depth_levels;
    return YGZF_OK;
}

int ygzf_bow_transform(ygzf_ctx *c, int n, const uint8_t *desc, int levelsup, int *leaf_node, int *level_node) {
    if (!c) return YGZF_ERR_INVALID;
    if (c->vocNodes < 1) return fail(c, YGZF_ERR_STATE, "no vocabulary on the device (ygzf_vocabulary_set)");
    if (n < 0) return fail(c, YGZF_ERR_INVALID, "negative count");
    if (n == 0) return YGZF_OK;
    if (!desc || !leaf_node || !level_node) return fail(c, YGZF_ERR_INVALID, "null argument");
    HIPCHECK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c, c->bow.desc, (size_t) n * 32)) || (rc = ensure(c, c->bow.leaf, (size_t) n * 4)) || (rc = ensure(c, c->bow.levelNode, (size_t) n * 4))) return rc;
    HIPCHECK(c, hipMemcpyAsync(c->bow.desc.p, desc, (size_t) n * 32, hipMemcpyHostToDevice, c->stream));
    {
        ProfScope ps(c, KK_BOW);
        launch_bow_descend(c->stream, n, (const uint8_t *) c->bow.desc.p, (const int *) c->voc.childOff.p, (const int *) c->voc.childIdx.p, (const uint8_t *) c->voc.nodeDesc.p,
                           c->vocLevels - levelsup, (int *) c->bow.leaf.p, (int *) c->bow.levelNode.p);
    }
    HIPCHECK(c, hipGetLastError());
    HIPCHECK(c, hipMemcpyAsync(leaf_node, c->bow.leaf.p, (size_t) n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipMemcpyAsync(level_node, c->bow.levelNode.p, (size_t) n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return YGZF_OK;
}

int ygzf_search_by_projection_kf(ygzf_ctx *c, const ygzf_frame_view *cur, const ygzf_camera *cam, int n_mp, const uint8_t *valid,
                                 const float *proj_x, const float *proj_y, const int *pred_level, const float *kf_angle, const uint8_t *mp_desc,
                                 float th, int orb_dist, int check_orientation, uint8_t *owner, int *match, int *nmatches) {
    if (!c || !cur || !owner) return fail(c, YGZF_ERR_INVALID, "null argument");
    if (orb_dist < 0 || orb_dist > 256) return fail(c, YGZF_ERR_INVALID, "ORBdist %d outside 0..256", orb_dist);
    for (int i = 0; i < cur->n; i++) owner[i] = owner[i] ? 2 : 0;   // `if (CurrentFrame.mvpMapPoints[i2]) continue;` (:1419): any MapPoint blocks
    ProjectedQuery Q = {};
    Q.mode = 2; Q.n_mp = n_mp;
    Q.track_in_view = valid;
    Q.proj_x = proj_x; Q.proj_y = proj_y; Q.mp_angle = kf_angle; Q.scale_level = pred_level;
    Q.mp_desc = mp_desc;
    Q.th = th; Q.max_dist = orb_dist; Q.check_ori = check_orientation;
    Q.owner = owner; Q.match = match; Q.nmatches = nmatches;
    return projected_match(c, cur, cam, Q);
}

}  // extern "C"
