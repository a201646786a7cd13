// ygzf_api_kfstore.hip -- the resident keyframes: what a KeyFrame never changes after its construction, put on the device once, with its grid
// built once (C ABI of libygzf, include/ygzf.h; product code: no CPU fallback, nothing from oracle/ is included or linked).  Kernel:
// kfstore_kernels.hip; state: ygzf_ctx::KfStore (ygzf_ctx.h); the searches that read the store: ygzf_api_match.hip.  The lifecycle follows the
// keyframe database's (ygzf_api_kfdb.hip): the host's slot table is the authority; every call validates first, does its device work, and
// commits the host state last, so an error leaves the store as it was.
#include <algorithm>

#include "ygzf_ctx.h"

extern "C" {

// room for `bytes` more at S.top.  When the row does not fit behind the last one the live rows move into a fresh arena in slot order, packed,
// device to device, and the holes of erased rows are gone.  The fresh arena is twice the size (doubling until everything fits) unless the live
// rows and the new one fill at most half of the present size: then it is of the same size, so that a store whose keyframes come and go stays
// bounded by its live rows.  Slot records hold offsets: nothing else moves.
static int kfs_reserve(ygzf_ctx *c, size_t bytes) {
    ygzf_ctx::KfStore &S = c->kfs;
    if (S.cap == 0) {
        size_t cap = YGZF_KF_INITIAL_BYTES;
        while (cap < bytes) cap *= 2;
        int rc = ensure(c, S.dArena, cap);
        if (rc) return rc;
        S.cap = cap;
        return YGZF_OK;
    }
    if (S.top + bytes <= S.cap) return YGZF_OK;
    size_t cap = S.liveBytes + bytes <= S.cap / 2 ? S.cap : S.cap * 2;
    while (S.liveBytes + bytes > cap) cap *= 2;
    ygzf_ctx::Buf fresh;   // (a local: it frees itself on the error returns below)
    int rc = ensure(c, fresh, cap);
    if (rc) return rc;
    const size_t n = S.slots.size();
    std::vector<long long> newOff(n, 0);
    size_t top = 0;
    hipError_t e = hipSuccess;
    for (size_t s = 0; s < n && e == hipSuccess; s++) {
        const ygzf_ctx::KfStore::Slot &L = S.slots[s];
        if (!L.live) continue;
        newOff[s] = (long long) top;
        e = hipMemcpyAsync((uint8_t *) fresh.p + top, (const uint8_t *) S.dArena.p + L.off, L.bytes, hipMemcpyDeviceToDevice, c->stream);
        top += L.bytes;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, YGZF_ERR_HIP, "repacking the keyframe store failed: %s", hipGetErrorString(e));
    S.dArena = std::move(fresh);   // the repack has completed: the old arena goes
    S.cap = cap;
    S.top = top;
    for (size_t s = 0; s < n; s++)
        if (S.slots[s].live) S.slots[s].off = newOff[s];
    return YGZF_OK;
}

int ygzf_kf_put(ygzf_ctx *c, uint64_t key, const ygzf_kf_static *kf, int *slot) {
    if (!c) return YGZF_ERR_INVALID;
    if (!kf) return fail(c, YGZF_ERR_INVALID, "null argument");
    int rc;
    if ((rc = kf_args_check(c, kf->view, kf->cam, kf->inv_level_sigma2, 0, false))) return rc;
    ygzf_ctx::KfStore &S = c->kfs;
    if (S.slotOf.count(key)) return fail(c, YGZF_ERR_STATE, "key %llu is already resident (slot %d)", (unsigned long long) key, S.slotOf[key]);
    if (S.freeSlots.empty() && S.slots.size() >= (size_t) std::numeric_limits<int>::max() / 2) return fail(c, YGZF_ERR_UNSUPPORTED, "too many slots");
    HIPCHECK(c, hipSetDevice(c->device));
    ygzf_ctx::KfStore::Slot L;
    kf_record_static(c, kf->view, kf->cam, kf->inv_level_sigma2, kf->log_scale_factor, L.kf);
    L.hasSigma = kf->inv_level_sigma2 != nullptr;
    // the row: the three arrays as the packed upload lays them out (one copy from the staging area), then the grid
    const size_t n = (size_t) kf->view.n;
    PackedTransfer P(c);
    L.kf.keys = (long long) P.add_in(kf->view.keys, sizeof(ygzf_kp) * n);
    L.kf.desc = (long long) P.add_in(kf->view.desc, 32 * n);
    L.kf.uRight = kf->view.u_right ? (long long) P.add_in(kf->view.u_right, 4 * n) : -1;
    L.cellStart = (long long) P.inBytes;
    L.list = L.cellStart + (long long) PackedTransfer::al(sizeof(int) * ((size_t) kKfGridCells + 1));
    L.bytes = (size_t) L.list + PackedTransfer::al(sizeof(int) * n);
    if ((rc = kfs_reserve(c, L.bytes))) return rc;
    L.off = (long long) S.top;
    uint8_t *row = (uint8_t *) S.dArena.p + S.top, *d;
    if ((rc = P.upload(&d))) return rc;
    if (P.inBytes) HIPCHECK(c, hipMemcpyAsync(row, d, P.inBytes, hipMemcpyDeviceToDevice, c->stream));
    KfGridArgs A;
    A.keys = (const ygzf_kp *) (row + L.kf.keys);
    A.n = (int) n;
    A.minX = L.kf.minX; A.minY = L.kf.minY; A.gridInvW = L.kf.gridInvW; A.gridInvH = L.kf.gridInvH;
    A.cellStart = (int *) (row + L.cellStart);
    A.list = (int *) (row + L.list);
    {
        ProfScope ps(c, KK_KFGRID);
        HIPCHECK(c, launch_kf_grid_build(c->stream, A));
    }
    HIPCHECK(c, hipGetLastError());
    HIPCHECK(c, hipStreamSynchronize(c->stream));   // the staging area and the caller's arrays are free again
    int s;
    if (S.freeSlots.empty()) {
        s = (int) S.slots.size();
        S.slots.emplace_back();
        S.keys.push_back(0);
    } else {
        s = *S.freeSlots.begin();
        S.freeSlots.erase(S.freeSlots.begin());
    }
    L.live = true;
    S.slots[s] = L;
    S.keys[s] = key;
    S.slotOf[key] = s;
    S.top += L.bytes;
    S.liveBytes += L.bytes;
    if (slot) *slot = s;
    return YGZF_OK;
}

int ygzf_kf_erase(ygzf_ctx *c, uint64_t key) {
    if (!c) return YGZF_ERR_INVALID;
    ygzf_ctx::KfStore &S = c->kfs;
    auto it = S.slotOf.find(key);
    if (it == S.slotOf.end()) return YGZF_OK;
    const int s = it->second;
    S.liveBytes -= S.slots[s].bytes;
    S.slots[s].live = false;
    S.freeSlots.insert(s);
    S.slotOf.erase(it);
    return YGZF_OK;
}

int ygzf_kf_clear(ygzf_ctx *c) {
    if (!c) return YGZF_ERR_INVALID;
    ygzf_ctx::KfStore &S = c->kfs;
    S.slots.clear();
    S.keys.clear();
    S.slotOf.clear();
    S.freeSlots.clear();
    S.top = S.liveBytes = 0;
    return YGZF_OK;
}

int ygzf_kf_has(ygzf_ctx *c, uint64_t key, int *has) {
    if (!c) return YGZF_ERR_INVALID;
    if (has) *has = c->kfs.slotOf.count(key) ? 1 : 0;
    return YGZF_OK;
}

int ygzf_kf_size(ygzf_ctx *c, int *n_live, int *n_slots) {
    if (!c) return YGZF_ERR_INVALID;
    if (n_live) *n_live = (int) c->kfs.slotOf.size();
    if (n_slots) *n_slots = (int) c->kfs.slots.size();
    return YGZF_OK;
}

int ygzf_kf_capacity(ygzf_ctx *c, size_t *bytes, size_t *used) {
    if (!c) return YGZF_ERR_INVALID;
    if (bytes) *bytes = c->kfs.cap ? c->kfs.cap : (size_t) YGZF_KF_INITIAL_BYTES;
    if (used) *used = c->kfs.top;
    return YGZF_OK;
}

int ygzf_kf_grid(ygzf_ctx *c, uint64_t key, int *cell_start, int *list) {
    if (!c) return YGZF_ERR_INVALID;
    const ygzf_ctx::KfStore &S = c->kfs;
    const auto it = S.slotOf.find(key);
    if (it == S.slotOf.end()) return fail(c, YGZF_ERR_INVALID, "key %llu is not resident", (unsigned long long) key);
    const ygzf_ctx::KfStore::Slot &L = S.slots[it->second];
    HIPCHECK(c, hipSetDevice(c->device));
    const uint8_t *row = (const uint8_t *) S.dArena.p + L.off;
    if (cell_start) HIPCHECK(c, hipMemcpyAsync(cell_start, row + L.cellStart, sizeof(int) * ((size_t) kKfGridCells + 1), hipMemcpyDeviceToHost, c->stream));
    if (list && L.kf.n > 0) HIPCHECK(c, hipMemcpyAsync(list, row + L.list, sizeof(int) * (size_t) L.kf.n, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return YGZF_OK;
}

}  // extern "C"
