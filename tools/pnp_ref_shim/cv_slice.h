// cv_slice.h -- the slice of OpenCV that the reference's src/PnPsolver.cc uses, for tools/make_golden_pnp_ref.py: a cv::Mat that can wrap
// caller memory, convert doubles to floats and copy into a view, and the C API calls of EPnP.  The four linear-algebra routines are NOT
// OpenCV's: they are this project's fixed text (csrc/pnp_math.h) run by one lane, so the record pins the reference's EPnP and RANSAC logic
// and roundings over that text, and nothing of the text itself.
#ifndef PNP_REF_CV_SLICE_H
#define PNP_REF_CV_SLICE_H
#include <cassert>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "pnp_math.h"

#define CV_32F 5
#define CV_64F 6
#define CV_SVD 1
#define CV_SVD_MODIFY_A 1
#define CV_SVD_U_T 2
#define CV_SVD_V_T 4

namespace cv {
struct Point2f { float x = 0, y = 0; };
struct Point3f {
    float x = 0, y = 0, z = 0;
    Point3f() {}
    Point3f(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
};
struct KeyPoint { Point2f pt; int octave = 0; };

class Mat {
public:
    int rows = 0, cols = 0, type = CV_32F;
    size_t step = 0;
    uint8_t *data = nullptr;
    Mat() {}
    Mat(int r, int c, int t) : rows(r), cols(c), type(t), step((size_t) c * es(t)), hold_(new std::vector<uint8_t>((size_t) r * c * es(t), 0)) { data = hold_->data(); }
    Mat(int r, int c, int t, void *user) : rows(r), cols(c), type(t), step((size_t) c * es(t)), data((uint8_t *) user) {}
    static size_t es(int t) { return t == CV_64F ? 8 : 4; }
    bool empty() const { return data == nullptr; }
    static Mat eye(int r, int c, int t) {
        assert(t == CV_32F);
        Mat m(r, c, t);
        for (int i = 0; i < r && i < c; i++) m.at<float>(i, i) = 1.f;
        return m;
    }
    template <class T> T &at(int y, int x) { return *(T *) (data + (size_t) y * step + (size_t) x * sizeof(T)); }
    template <class T> const T &at(int y, int x) const { return *(const T *) (data + (size_t) y * step + (size_t) x * sizeof(T)); }
    template <class T> T &at(int i) { return at<T>(i, 0); }
    template <class T> const T &at(int i) const { return at<T>(i, 0); }
    void convertTo(Mat &dst, int t) const {   // (dst may be *this)
        assert(type == CV_64F && t == CV_32F);
        Mat o(rows, cols, CV_32F);
        for (int y = 0; y < rows; y++)
            for (int x = 0; x < cols; x++) o.at<float>(y, x) = (float) at<double>(y, x);
        dst = o;
    }
    Mat rowRange(int a, int b) const { Mat m = *this; m.data = data + (size_t) a * step; m.rows = b - a; return m; }
    Mat colRange(int a, int b) const { Mat m = *this; m.data = data + (size_t) a * es(type); m.cols = b - a; return m; }
    Mat col(int i) const { return colRange(i, i + 1); }
    void copyTo(const Mat &dst) const {   // into a view of the same shape
        assert(dst.rows == rows && dst.cols == cols && dst.type == type);
        for (int y = 0; y < rows; y++) std::memcpy(dst.data + (size_t) y * dst.step, data + (size_t) y * step, (size_t) cols * es(type));
    }
    Mat clone() const {
        if (empty()) return Mat();
        Mat o(rows, cols, type);
        copyTo(o);
        return o;
    }
private:
    std::shared_ptr<std::vector<uint8_t>> hold_;
};
}  // namespace cv

struct CvMat {
    int rows, cols;
    union { double *db; } data;
};
inline CvMat cvMat(int r, int c, int, void *p) { CvMat m; m.rows = r; m.cols = c; m.data.db = (double *) p; return m; }
inline CvMat *cvCreateMat(int r, int c, int) { CvMat *m = new CvMat; m->rows = r; m->cols = c; m->data.db = new double[(size_t) r * c]; return m; }
inline void cvReleaseMat(CvMat **m) { delete[] (*m)->data.db; delete *m; *m = nullptr; }
inline void cvmSet(CvMat *m, int r, int c, double v) { m->data.db[(size_t) r * m->cols + c] = v; }
inline double cvmGet(const CvMat *m, int r, int c) { return m->data.db[(size_t) r * m->cols + c]; }
inline void cvSetZero(CvMat *m) { for (int i = 0; i < m->rows * m->cols; i++) m->data.db[i] = 0.0; }

namespace pnp_ref {
const ygzf::pnp::Lanes kOne = {0, 1};
inline std::vector<double> transposed(const CvMat *A) {
    std::vector<double> At((size_t) A->rows * A->cols);
    for (int r = 0; r < A->rows; r++)
        for (int c = 0; c < A->cols; c++) At[(size_t) c * A->rows + r] = A->data.db[(size_t) r * A->cols + c];
    return At;
}
}  // namespace pnp_ref

// dst = src' src: every entry of the upper triangle summed over the rows in order, mirrored (csrc/pnp_math.h states the form)
inline void cvMulTransposed(const CvMat *src, CvMat *dst, int order) {
    assert(order == 1 && dst->rows == src->cols && dst->cols == src->cols);
    const int n = src->cols;
    for (int i = 0; i < n; i++)
        for (int j = i; j < n; j++) {
            double s = 0;
            for (int r = 0; r < src->rows; r++) s += src->data.db[(size_t) r * n + i] * src->data.db[(size_t) r * n + j];
            dst->data.db[(size_t) i * n + j] = dst->data.db[(size_t) j * n + i] = s;
        }
}
inline void cvSVD(CvMat *A, CvMat *W, CvMat *U, CvMat *V, int flags) {
    const int m = A->rows, n = A->cols;
    assert(m >= n && !(flags & CV_SVD_V_T));
    std::vector<double> At = pnp_ref::transposed(A), w(n), Vt((size_t) n * n);
    ygzf::pnp::jacobi_svd(At.data(), m, w.data(), V ? Vt.data() : nullptr, n, m, n, pnp_ref::kOne);
    for (int i = 0; i < n; i++) W->data.db[i] = w[i];
    if (U)
        for (int i = 0; i < n; i++)
            for (int k = 0; k < m; k++) {
                if (flags & CV_SVD_U_T) U->data.db[(size_t) i * m + k] = At[(size_t) i * m + k];
                else U->data.db[(size_t) k * n + i] = At[(size_t) i * m + k];
            }
    if (V)
        for (int j = 0; j < n; j++)
            for (int k = 0; k < n; k++) V->data.db[(size_t) j * n + k] = Vt[(size_t) k * n + j];
}
inline int cvSolve(const CvMat *A, const CvMat *b, CvMat *x, int method) {
    assert(method == CV_SVD);
    const int m = A->rows, n = A->cols;
    std::vector<double> At = pnp_ref::transposed(A), w(n), Vt((size_t) n * n);
    ygzf::pnp::solve_svd(At.data(), w.data(), Vt.data(), m, n, b->data.db, x->data.db, pnp_ref::kOne);
    return 1;
}
inline double cvInvert(const CvMat *A, CvMat *inv, int method) {
    assert(method == CV_SVD && A->rows == 3 && A->cols == 3);
    std::vector<double> At = pnp_ref::transposed(A);
    double w[3], Vt[9];
    ygzf::pnp::invert3_svd(At.data(), w, Vt, inv->data.db, pnp_ref::kOne);
    return 1;
}
#endif
