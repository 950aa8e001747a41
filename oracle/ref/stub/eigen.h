// Stand-in for the Eigen header the firmware's ekf.h includes: the dozen operations of dynamic double matrices that
// ekf.cpp uses, and nothing else.  TEST INFRASTRUCTURE ONLY (oracle/ref/Makefile builds the firmware's own ekf.cpp against it).
//
// One class serves as MatrixXd and as VectorXd (a vector is an n x 1 matrix).  Every product is a triple loop that starts
// its sum at 0.0 and adds the terms in ascending k; A * B * C evaluates left to right, as C++ parses it; sums and
// differences are element by element; inverse() is the 2 x 2 adjugate times (1 / det).  No expression templates, no
// vectorisation, no fused multiply-add (built with -ffp-contract=off): one rounding per written operation.
#ifndef QS_REF_EIGEN_STANDIN_H
#define QS_REF_EIGEN_STANDIN_H

#include <cassert>
#include <cstddef>
#include <vector>

namespace Eigen {

class Mat;

class CommaInit {                                  // m << a, b, c: fills in storage order of the target (row-major matrix, or diagonal)
public:
    CommaInit(Mat *m, bool diag, double first) : m_(m), diag_(diag), at_(0) { put(first); }
    CommaInit &operator,(double v) { put(v); return *this; }
private:
    void put(double v);
    Mat *m_; bool diag_; int at_;
};

class DiagRef {
public:
    explicit DiagRef(Mat *m) : m_(m) {}
    CommaInit operator<<(double v) { return CommaInit(m_, true, v); }
private:
    Mat *m_;
};

class Mat {
public:
    Mat() : r_(0), c_(0) {}
    explicit Mat(int n) : r_(n), c_(1), d_((size_t)n, 0.0) {}
    Mat(int r, int c) : r_(r), c_(c), d_((size_t)r * c, 0.0) {}

    static Mat Zero(int n) { return Mat(n); }
    static Mat Zero(int r, int c) { return Mat(r, c); }
    static Mat Identity(int r, int c) { Mat m(r, c); for (int i = 0; i < r && i < c; i++) m(i, i) = 1.0; return m; }

    int rows() const { return r_; }
    int cols() const { return c_; }
    double &operator()(int i) { assert(c_ == 1); return d_[(size_t)i]; }
    double operator()(int i) const { assert(c_ == 1); return d_[(size_t)i]; }
    double &operator()(int i, int j) { return d_[(size_t)i * c_ + j]; }
    double operator()(int i, int j) const { return d_[(size_t)i * c_ + j]; }

    DiagRef diagonal() { return DiagRef(this); }
    CommaInit operator<<(double v) { return CommaInit(this, false, v); }

    Mat transpose() const { Mat t(c_, r_); for (int i = 0; i < r_; i++) for (int j = 0; j < c_; j++) t(j, i) = (*this)(i, j); return t; }
    Mat inverse() const
    {
        assert(r_ == 2 && c_ == 2);
        const Mat &s = *this;
        const double det = s(0, 0) * s(1, 1) - s(0, 1) * s(1, 0);
        const double invdet = 1.0 / det;
        Mat o(2, 2);
        o(0, 0) = s(1, 1) * invdet; o(0, 1) = -s(0, 1) * invdet;
        o(1, 0) = -s(1, 0) * invdet; o(1, 1) = s(0, 0) * invdet;
        return o;
    }

private:
    int r_, c_;
    std::vector<double> d_;
};

inline void CommaInit::put(double v)
{
    if (diag_) { (*m_)(at_, at_) = v; at_++; }
    else { (*m_)(at_ / m_->cols(), at_ % m_->cols()) = v; at_++; }
}

inline Mat operator*(const Mat &a, const Mat &b)
{
    assert(a.cols() == b.rows());
    Mat o(a.rows(), b.cols());
    for (int i = 0; i < a.rows(); i++)
        for (int j = 0; j < b.cols(); j++) {
            double s = 0.0;
            for (int k = 0; k < a.cols(); k++) s += a(i, k) * b(k, j);
            o(i, j) = s;
        }
    return o;
}
inline Mat operator+(const Mat &a, const Mat &b)
{
    assert(a.rows() == b.rows() && a.cols() == b.cols());
    Mat o(a.rows(), a.cols());
    for (int i = 0; i < a.rows(); i++) for (int j = 0; j < a.cols(); j++) o(i, j) = a(i, j) + b(i, j);
    return o;
}
inline Mat operator-(const Mat &a, const Mat &b)
{
    assert(a.rows() == b.rows() && a.cols() == b.cols());
    Mat o(a.rows(), a.cols());
    for (int i = 0; i < a.rows(); i++) for (int j = 0; j < a.cols(); j++) o(i, j) = a(i, j) - b(i, j);
    return o;
}

typedef Mat MatrixXd;
typedef Mat VectorXd;

}  // namespace Eigen

#endif
