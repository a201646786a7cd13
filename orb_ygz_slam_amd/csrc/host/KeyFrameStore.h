// KeyFrameStore.h -- ygz::KeyFrameDeviceStore: the keyframes the Fuse shells have met, resident on the device (include/ygzf.h: ygzf_kf_put and
// the resident searches).  What a KeyFrame never changes after its construction -- mvKeys, mDescriptors, mvuRight, the scale tables, the
// calibration, the bounds and the grid -- goes up once; every later Fuse against it sends its pose and the points.
//   One store per device, with one context of its own and a mutex: every use holds the mutex for the whole device call.
//   Keyed by the KeyFrame's address.  The store remembers mnId and N per entry and puts again when they differ, which covers an address that
//   comes back with another keyframe (Tracking::Reset deletes the map and restarts the id counter).
//   Off by default: with sResident false ORBmatcher::Fuse, ygz::FuseBatch, ORBmatcher::Fuse(pKF, Scw, ..) and ygz::SearchAndFuseBatch send the
//   keyframes with every call, as before.  With it true they put each target they meet and search the resident copies; results are the same bits.
//   The caller's duties: Erase where the keyframe goes bad (KeyFrame::SetBadFlag), Clear in Tracking::Reset.  An entry whose
//   keyframe was deleted without Erase only wastes memory until its address is reused, when the mnId check replaces it.
// Everything the matcher shells use is defined here, so that ORBmatcherFuse.cc and ORBmatcherLoop.cc link as before; KeyFrameStore.cc adds
// Put(KeyFrame *) for callers that want a keyframe resident ahead of its first Fuse.
#ifndef YGZF_KEYFRAME_STORE_H
#define YGZF_KEYFRAME_STORE_H
#include <cstdint>
#include <map>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "../../../include/ygzf.h"
#include "ygzf_pool.h"

namespace ygz {
class KeyFrame;

class KeyFrameDeviceStore {
public:
    inline static bool sResident = false;          // the switch (read at every call, like ORBextractor::sDevice)
    struct Statistics {
        unsigned long puts = 0, hits = 0, queries = 0;   // keyframes uploaded / found resident / device searches run through the store
        unsigned long long bytesUploaded = 0;            // keys + descriptors + mvuRight of the puts
    };
    static KeyFrameDeviceStore &instance(int device) {   // created on first use, never destroyed (ygzf_pool.h says why)
        static std::mutex mu;
        static std::map<int, KeyFrameDeviceStore *> *stores = new std::map<int, KeyFrameDeviceStore *>();
        std::lock_guard<std::mutex> lk(mu);
        KeyFrameDeviceStore *&s = (*stores)[device];
        if (!s) s = new KeyFrameDeviceStore(device);
        return *s;
    }

    bool Put(KeyFrame *pKF);      // (KeyFrameStore.cc) resident when it returns true, a hit when it already was; false: ygzf_host::report_failure has it
    void Erase(KeyFrame *pKF) {   // unknown keyframe: nothing
        std::lock_guard<std::mutex> lk(mu_);
        if (entries_.erase(pKF) && ctx_) ygzf_kf_erase(ctx_, key(pKF));
    }
    void Clear() {                // no keyframes; the device memory is kept
        std::lock_guard<std::mutex> lk(mu_);
        entries_.clear();
        if (ctx_) ygzf_kf_clear(ctx_);
    }
    void Release() {              // ... and the device memory and the context are freed (the next put creates them again)
        std::lock_guard<std::mutex> lk(mu_);
        entries_.clear();
        if (ctx_) ygzf_destroy(ctx_);
        ctx_ = nullptr;
    }
    Statistics Stats() {
        std::lock_guard<std::mutex> lk(mu_);
        return stats_;
    }
    static uint64_t key(const KeyFrame *pKF) { return (uint64_t) (uintptr_t) pKF; }

    // The shells' access: locks the store for the caller's scope.
    class Guard {
    public:
        explicit Guard(KeyFrameDeviceStore &s) : s_(s), lk_(s.mu_) {}
        ygzf_ctx *ctx(const char *who) { return s_.ensure_ctx(who) ? s_.ctx_ : nullptr; }
        // the keyframe at pKF with this mnId and N is resident afterwards; pack(rec, hold) fills its arrays and is called on a miss only
        template <class Pack>
        bool resident(const KeyFrame *pKF, unsigned long mnId, int N, Pack &&pack, const char *who) {
            KeyFrameDeviceStore &S = s_;
            if (!pKF || !S.ensure_ctx(who)) return false;
            auto it = S.entries_.find(pKF);
            if (it != S.entries_.end()) {
                if (it->second.mnId == mnId && it->second.N == N) {
                    S.stats_.hits++;
                    return true;
                }
                ygzf_kf_erase(S.ctx_, key(pKF));   // another keyframe at this address
                S.entries_.erase(it);
            }
            ygzf_kf_static rec;
            std::vector<uint8_t> hold;
            if (!pack(rec, hold)) return false;
            if (ygzf_kf_put(S.ctx_, key(pKF), &rec, nullptr) != YGZF_OK) {
                ygzf_host::report_failure(who, ygzf_last_error(S.ctx_));
                return false;
            }
            S.entries_[pKF] = Entry{mnId, N};
            S.stats_.puts++;
            S.stats_.bytesUploaded += (unsigned long long) (rec.view.n > 0 ? rec.view.n : 0) * (sizeof(ygzf_kp) + 32 + (rec.view.u_right ? 4 : 0));
            return true;
        }
        void count_query() { s_.stats_.queries++; }

    private:
        KeyFrameDeviceStore &s_;
        std::lock_guard<std::mutex> lk_;
    };

private:
    explicit KeyFrameDeviceStore(int device) : device_(device) {}
    bool ensure_ctx(const char *who) {
        if (ctx_) return true;
        // Only the context's stream, staging area and keyframe store are used (as the keyframe database's context, host/KeyFrameDatabase.cc).
        ygzf_extractor_cfg cfg = {1000, 1.2f, 8, 20, 7, 0};
        if (ygzf_create(device_, &cfg, 64, 64, 1, &ctx_) != YGZF_OK) {
            ygzf_host::report_failure(who, ygzf_last_error(nullptr));
            ctx_ = nullptr;
            return false;
        }
        return true;
    }
    struct Entry { unsigned long mnId; int N; };
    int device_;
    ygzf_ctx *ctx_ = nullptr;
    std::mutex mu_;
    std::unordered_map<const KeyFrame *, Entry> entries_;
    Statistics stats_;
};
}  // namespace ygz
#endif
