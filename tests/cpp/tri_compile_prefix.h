// tri_compile_prefix.h -- tests/test_tri_shell_compiles.py: the real include/KeyFrame.h needs Eigen and Sophus, so the compile check of
// host/LocalMappingTriangulate.cc runs over the stand-in KeyFrame of oracle/ref_shim/matcher_stubs.h, which has every member
// LocalMapping::CreateNewMapPoints reads but four: mvDepth, invfx, invfy and mfScaleFactor (include/KeyFrame.h:289-310).  They are declared here
// with the real header's types, into the stand-in's own member lists, by reading that header once with two of its member names widened.
#define mvuRight mvuRight, mvDepth
#define mfLogScaleFactor mfLogScaleFactor = 0, invfx = 0, invfy = 0, mfScaleFactor
#include "mini_cv.h"
#undef mvuRight
#undef mfLogScaleFactor
