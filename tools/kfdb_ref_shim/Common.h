// tools/kfdb_ref_shim/Common.h -- TEST INFRASTRUCTURE of tools/make_golden_kfdb_ref.py: what the reference's src/KeyFrameDatabase.cc and
// include/KeyFrameDatabase.h take from their Common.h -- the standard containers, `using namespace std` and glog's LOG(INFO) as a sink.  Carries
// the reference header's guard, so that the real one (found first beside KeyFrameDatabase.h) stays out once this one is force-included.
#ifndef YGZ_COMMON_H_
#define YGZ_COMMON_H_
#include <algorithm>
#include <iostream>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <vector>

using namespace std;

struct KfdbNullLog {
    template <class T> KfdbNullLog &operator<<(const T &) { return *this; }
    KfdbNullLog &operator<<(std::ostream &(*)(std::ostream &)) { return *this; }
};
#define LOG(severity) KfdbNullLog()
#endif
