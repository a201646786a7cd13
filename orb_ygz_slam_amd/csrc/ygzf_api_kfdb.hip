// ygzf_api_kfdb.hip -- KeyFrameDatabase: the device-resident BowVector store and its query (C ABI of libygzf, include/ygzf.h; product code: no
// CPU fallback, nothing from oracle/ is included or linked).  Kernels: kfdb_kernels.hip; state: ygzf_ctx::Kfdb (ygzf_ctx.h).  The host's slot
// table is the authority; every call validates first, does its device work, and commits the host state last, so an error leaves the store as it was.
#include <algorithm>

#include "ygzf_ctx.h"

extern "C" {

static void kfdb_mark_dirty(ygzf_ctx::Kfdb &K, int lo, int hi) {
    if (K.dirtyLo == K.dirtyHi) { K.dirtyLo = lo; K.dirtyHi = hi; return; }
    K.dirtyLo = std::min(K.dirtyLo, lo);
    K.dirtyHi = std::max(K.dirtyHi, hi);
}

// a fresh arena of `entries` entries in two buffers of the caller's: a local Buf that does not reach the context frees itself
static int kfdb_alloc_arena(ygzf_ctx *c, size_t entries, ygzf_ctx::Buf &ids, ygzf_ctx::Buf &vals) {
    int rc;
    if ((rc = ensure(c, ids, sizeof(uint32_t) * entries)) || (rc = ensure(c, vals, sizeof(double) * entries))) return rc;
    return YGZF_OK;
}

// room for n more entries at K.top.  When the row does not fit behind the last one the live rows move into a fresh arena in slot order, packed,
// by one kernel, and the holes of erased rows are gone.  The fresh arena is twice the size (doubling until everything fits) unless the live
// rows and the new one fill at most half of the present size: then it is of the same size, so that a store whose keyframes come and go stays
// bounded by its live entries and not by everything ever appended.
static int kfdb_reserve(ygzf_ctx *c, size_t n) {
    ygzf_ctx::Kfdb &K = c->kfdb;
    int rc;
    if (K.cap == 0) {
        size_t cap = YGZF_KFDB_INITIAL_ENTRIES;
        while (cap < n) cap *= 2;
        if ((rc = kfdb_alloc_arena(c, cap, K.dIds, K.dVals))) return rc;
        K.cap = cap;
        return YGZF_OK;
    }
    if (K.top + n <= K.cap) return YGZF_OK;
    size_t cap = K.liveEntries + n <= K.cap / 2 ? K.cap : K.cap * 2;
    while (K.liveEntries + n > cap) cap *= 2;
    const size_t S = K.slots.size();
    std::vector<long long> newOff(S, 0);
    size_t top = 0;
    for (size_t s = 0; s < S; s++)
        if (K.slots[s].live) { newOff[s] = (long long) top; top += (size_t) K.slots[s].len; }
    ygzf_ctx::Buf ids, vals;
    if ((rc = kfdb_alloc_arena(c, cap, ids, vals))) return rc;
    if (top > 0) {
        PackedTransfer P(c);
        const size_t iT = P.add_in(K.slots.data(), sizeof(KfdbSlot) * S), iO = P.add_in(newOff.data(), sizeof(long long) * S);
        uint8_t *d;
        if ((rc = P.upload(&d))) return rc;
        launch_kfdb_repack(c->stream, (int) S, (const KfdbSlot *) (d + iT), (const long long *) (d + iO), (const unsigned *) K.dIds.p, (const double *) K.dVals.p,
                           (unsigned *) ids.p, (double *) vals.p);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(c, YGZF_ERR_HIP, "repacking the keyframe database failed: %s", hipGetErrorString(e));
    } else {
        HIPCHECK(c, hipStreamSynchronize(c->stream));
    }
    K.dIds = std::move(ids);     // the repack has completed: the old arena goes
    K.dVals = std::move(vals);
    K.cap = cap;
    K.top = top;
    for (size_t s = 0; s < S; s++)
        if (K.slots[s].live) K.slots[s].off = newOff[s];
    if (S) kfdb_mark_dirty(K, 0, (int) S);
    return YGZF_OK;
}

int ygzf_kfdb_add(ygzf_ctx *c, uint64_t key, int n, const uint32_t *ids, const double *vals, int *slot) {
    if (!c) return YGZF_ERR_INVALID;
    if (n < 0) return fail(c, YGZF_ERR_INVALID, "negative count");
    if (n > 0 && (!ids || !vals)) return fail(c, YGZF_ERR_INVALID, "null array");
    for (int i = 1; i < n; i++)
        if (ids[i] <= ids[i - 1]) return fail(c, YGZF_ERR_INVALID, "word ids not strictly ascending at entry %d", i);
    if (n > 0 && ids[n - 1] > kKfdbMaxWordId) return fail(c, YGZF_ERR_INVALID, "word id %u is above 2^31 - 1", ids[n - 1]);
    ygzf_ctx::Kfdb &K = c->kfdb;
    if (K.slotOf.count(key)) return fail(c, YGZF_ERR_STATE, "key %llu is already in the keyframe database (slot %d)", (unsigned long long) key, K.slotOf[key]);
    if (K.freeSlots.empty() && K.slots.size() >= (size_t) std::numeric_limits<int>::max() / 2) return fail(c, YGZF_ERR_UNSUPPORTED, "too many slots");
    HIPCHECK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = kfdb_reserve(c, (size_t) n))) return rc;
    if (n > 0) {
        PackedTransfer P(c);
        const size_t iI = P.add_in(ids, sizeof(uint32_t) * (size_t) n), iV = P.add_in(vals, sizeof(double) * (size_t) n);
        uint8_t *d;
        if ((rc = P.upload(&d))) return rc;
        HIPCHECK(c, hipMemcpyAsync((uint32_t *) K.dIds.p + K.top, d + iI, sizeof(uint32_t) * (size_t) n, hipMemcpyDeviceToDevice, c->stream));
        HIPCHECK(c, hipMemcpyAsync((double *) K.dVals.p + K.top, d + iV, sizeof(double) * (size_t) n, hipMemcpyDeviceToDevice, c->stream));
        HIPCHECK(c, hipStreamSynchronize(c->stream));   // the staging area and the caller's arrays are free again
    }
    int s;
    if (K.freeSlots.empty()) {
        s = (int) K.slots.size();
        K.slots.push_back(KfdbSlot{0, 0, 0});
        K.keys.push_back(0);
    } else {
        s = *K.freeSlots.begin();
        K.freeSlots.erase(K.freeSlots.begin());
    }
    K.slots[s] = KfdbSlot{(long long) K.top, n, 1};
    K.keys[s] = key;
    K.slotOf[key] = s;
    K.top += (size_t) n;
    K.liveEntries += (size_t) n;
    kfdb_mark_dirty(K, s, s + 1);
    if (slot) *slot = s;
    return YGZF_OK;
}

int ygzf_kfdb_erase(ygzf_ctx *c, uint64_t key) {
    if (!c) return YGZF_ERR_INVALID;
    ygzf_ctx::Kfdb &K = c->kfdb;
    auto it = K.slotOf.find(key);
    if (it == K.slotOf.end()) return YGZF_OK;
    const int s = it->second;
    K.liveEntries -= (size_t) K.slots[s].len;
    K.slots[s].live = 0;
    K.freeSlots.insert(s);
    K.slotOf.erase(it);
    kfdb_mark_dirty(K, s, s + 1);
    return YGZF_OK;
}

int ygzf_kfdb_clear(ygzf_ctx *c) {
    if (!c) return YGZF_ERR_INVALID;
    ygzf_ctx::Kfdb &K = c->kfdb;
    K.slots.clear();
    K.keys.clear();
    K.slotOf.clear();
    K.freeSlots.clear();
    K.top = K.liveEntries = 0;
    K.dirtyLo = K.dirtyHi = 0;
    return YGZF_OK;
}

int ygzf_kfdb_size(ygzf_ctx *c, int *n_live, int *n_slots) {
    if (!c) return YGZF_ERR_INVALID;
    if (n_live) *n_live = (int) c->kfdb.slotOf.size();
    if (n_slots) *n_slots = (int) c->kfdb.slots.size();
    return YGZF_OK;
}

int ygzf_kfdb_capacity(ygzf_ctx *c, size_t *entries, size_t *used) {
    if (!c) return YGZF_ERR_INVALID;
    if (entries) *entries = c->kfdb.cap ? c->kfdb.cap : (size_t) YGZF_KFDB_INITIAL_ENTRIES;
    if (used) *used = c->kfdb.top;
    return YGZF_OK;
}

int ygzf_kfdb_query(ygzf_ctx *c, int n_q, const ygzf_kfdb_query_vec *q, int *common, int *first, double *score) {
    if (!c) return YGZF_ERR_INVALID;
    if (n_q < 0) return fail(c, YGZF_ERR_INVALID, "negative count");
    ygzf_ctx::Kfdb &K = c->kfdb;
    const size_t S = K.slots.size(), Q = (size_t) n_q;
    if (Q * S == 0) return YGZF_OK;
    if (!q || !common || !first || !score) return fail(c, YGZF_ERR_INVALID, "null argument");
    for (size_t i = 0; i < Q * S; i++) { common[i] = 0; first[i] = -1; score[i] = 0.0; }
    std::vector<int> qOff(Q + 1, 0);
    int maxWords = 0;
    for (size_t k = 0; k < Q; k++) {
        if (q[k].n < 0) return fail(c, YGZF_ERR_INVALID, "query %zu: negative count", k);
        if (q[k].n > kKfdbMaxQueryWords) return fail(c, YGZF_ERR_UNSUPPORTED, "query %zu: %d words (at most %d)", k, q[k].n, kKfdbMaxQueryWords);
        if (q[k].n > 0 && (!q[k].ids || !q[k].vals)) return fail(c, YGZF_ERR_INVALID, "query %zu: null array", k);
        for (int i = 1; i < q[k].n; i++)
            if (q[k].ids[i] <= q[k].ids[i - 1]) return fail(c, YGZF_ERR_INVALID, "query %zu: word ids not strictly ascending at entry %d", k, i);
        if (q[k].n > 0 && q[k].ids[q[k].n - 1] > kKfdbMaxWordId) return fail(c, YGZF_ERR_INVALID, "query %zu: word id %u is above 2^31 - 1", k, q[k].ids[q[k].n - 1]);
        if ((long long) qOff[k] + q[k].n > std::numeric_limits<int>::max()) return fail(c, YGZF_ERR_UNSUPPORTED, "too many query words in one call");
        qOff[k + 1] = qOff[k] + q[k].n;
        maxWords = std::max(maxWords, q[k].n);
    }
    if (Q > 65535) return fail(c, YGZF_ERR_UNSUPPORTED, "more than 65535 queries in one call");
    HIPCHECK(c, hipSetDevice(c->device));
    const size_t W = (size_t) qOff[Q];
    std::vector<uint32_t> ids(W ? W : 1);
    std::vector<double> vals(W ? W : 1);
    for (size_t k = 0; k < Q; k++)
        if (q[k].n > 0) {
            memcpy(ids.data() + qOff[k], q[k].ids, sizeof(uint32_t) * (size_t) q[k].n);
            memcpy(vals.data() + qOff[k], q[k].vals, sizeof(double) * (size_t) q[k].n);
        }
    int rc;
    if (sizeof(KfdbSlot) * S > K.dTable.bytes) {   // (a table that moves has lost its contents: all of it goes again)
        size_t bytes = std::max<size_t>(K.dTable.bytes, sizeof(KfdbSlot) * 1024);
        while (bytes < sizeof(KfdbSlot) * S) bytes *= 2;
        if ((rc = ensure(c, K.dTable, bytes))) return rc;
        K.dirtyLo = 0;
        K.dirtyHi = (int) S;
    }
    K.dirtyHi = std::min(K.dirtyHi, (int) S);
    const size_t nDirty = K.dirtyHi > K.dirtyLo ? (size_t) (K.dirtyHi - K.dirtyLo) : 0;
    PackedTransfer P(c);
    const size_t iO = P.add_in(qOff.data(), sizeof(int) * (Q + 1)), iI = P.add_in(ids.data(), sizeof(uint32_t) * W), iV = P.add_in(vals.data(), sizeof(double) * W),
                 iT = P.add_in(K.slots.data() + K.dirtyLo, sizeof(KfdbSlot) * nDirty);
    const size_t oC = P.add_out(common, sizeof(int) * Q * S), oF = P.add_out(first, sizeof(int) * Q * S), oS = P.add_out(score, sizeof(double) * Q * S);
    uint8_t *d;
    if ((rc = P.upload(&d))) return rc;
    if (nDirty) {
        HIPCHECK(c, hipMemcpyAsync((KfdbSlot *) K.dTable.p + K.dirtyLo, d + iT, sizeof(KfdbSlot) * nDirty, hipMemcpyDeviceToDevice, c->stream));
        K.dirtyLo = K.dirtyHi = 0;
    }
    KfdbQueryArgs A;
    A.nSlots = (int) S;
    A.slots = (const KfdbSlot *) K.dTable.p;
    A.ids = (const unsigned *) K.dIds.p;
    A.vals = (const double *) K.dVals.p;
    A.qOff = (const int *) (d + iO);
    A.qIds = (const unsigned *) (d + iI);
    A.qVals = (const double *) (d + iV);
    A.common = (int *) P.d_out(oC);
    A.first = (int *) P.d_out(oF);
    A.score = (double *) P.d_out(oS);
    {
        ProfScope ps(c, KK_KFDB);
        launch_kfdb_query(c->stream, A, n_q, maxWords, c->cuCount);
    }
    HIPCHECK(c, hipGetLastError());
    return P.download();
}

}  // extern "C"
