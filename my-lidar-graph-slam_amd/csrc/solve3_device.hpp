// solve3_device.hpp -- the 3x3 column-pivoting Householder QR solve shared by
// the Gauss-Newton kernels (k_linsolve.hip, k_icp.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>

namespace lgs {

// Eigen ColPivHouseholderQR<Matrix3d>::compute + solve (published algorithm,
// Eigen >= 3.3), one thread.  Every loop is unrolled and every data-dependent
// index (pivot column, permutation) is resolved with compile-time-indexed
// selects, so the 3x3 problem lives in registers (no scratch).
template <class T>
__device__ __forceinline__ void cswap(bool c, T& a, T& b)
{
    const T ta = a, tb = b;
    a = c ? tb : ta;
    b = c ? ta : tb;
}

__device__ inline void solve3_colpiv_qr(const double Hin[9], const double bin[3], double xout[3])
{
    constexpr int N = 3;
    double A[N][N];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) A[i][j] = Hin[3 * i + j];
    double hc[N], normU[N], normD[N];
    int transp[N];
    const double eps = DBL_EPSILON;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) s += A[i][k] * A[i][k];
        normD[k] = sqrt(s);
        normU[k] = normD[k];
    }
    double maxn = normU[0];
#pragma unroll
    for (int k = 1; k < N; ++k)
        if (normU[k] > maxn) maxn = normU[k];
    const double thrHelper = (maxn * eps) * (maxn * eps) / (double)N;
    const double downdateThr = sqrt(eps);
    int nonzero = N;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        int big = k;
        double bigv = normU[k];
#pragma unroll
        for (int j = k + 1; j < N; ++j)
            if (normU[j] > bigv) {
                bigv = normU[j];
                big = j;
            }
        if (nonzero == N && bigv * bigv < thrHelper * (double)(N - k)) nonzero = k;
        transp[k] = big;
#pragma unroll
        for (int j = k + 1; j < N; ++j) {
            const bool sw = (j == big);
#pragma unroll
            for (int i = 0; i < N; ++i) cswap(sw, A[i][k], A[i][j]);
            cswap(sw, normU[k], normU[j]);
            cswap(sw, normD[k], normD[j]);
        }
        double tailSq = 0.0;
#pragma unroll
        for (int i = k + 1; i < N; ++i) tailSq += A[i][k] * A[i][k];
        const double c0 = A[k][k];
        double tau, beta;
        if (tailSq <= DBL_MIN) {
            tau = 0.0;
            beta = c0;
#pragma unroll
            for (int i = k + 1; i < N; ++i) A[i][k] = 0.0;
        } else {
            beta = sqrt(c0 * c0 + tailSq);
            if (c0 >= 0.0) beta = -beta;
#pragma unroll
            for (int i = k + 1; i < N; ++i) A[i][k] = A[i][k] / (c0 - beta);
            tau = (beta - c0) / beta;
        }
        hc[k] = tau;
        A[k][k] = beta;
        if (tau != 0.0) {
#pragma unroll
            for (int j = k + 1; j < N; ++j) {
                double tmp = 0.0;
#pragma unroll
                for (int i = k + 1; i < N; ++i) tmp += A[i][k] * A[i][j];
                tmp += A[k][j];
                A[k][j] -= tau * tmp;
#pragma unroll
                for (int i = k + 1; i < N; ++i) A[i][j] -= (tau * A[i][k]) * tmp;
            }
        }
#pragma unroll
        for (int j = k + 1; j < N; ++j) {
            if (normU[j] != 0.0) {
                double temp = fabs(A[k][j]) / normU[j];
                temp = (1.0 + temp) * (1.0 - temp);
                temp = temp < 0.0 ? 0.0 : temp;
                const double q = normU[j] / normD[j];
                if (temp * (q * q) <= downdateThr) {
                    double s = 0.0;
#pragma unroll
                    for (int i = k + 1; i < N; ++i) s += A[i][j] * A[i][j];
                    normD[j] = sqrt(s);
                    normU[j] = normD[j];
                } else {
                    normU[j] *= sqrt(temp);
                }
            }
        }
    }
    // permutation: perm = transpositions applied in order
    int perm[N] = { 0, 1, 2 };
#pragma unroll
    for (int k = 0; k < N; ++k)
#pragma unroll
        for (int j = k + 1; j < N; ++j) cswap(transp[k] == j, perm[k], perm[j]);
    if (nonzero == 0) {
        xout[0] = xout[1] = xout[2] = 0.0;
        return;
    }
    double c[N] = { bin[0], bin[1], bin[2] };
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if (k >= nonzero) break;
        if (k == N - 1) {
            c[k] *= 1.0 - hc[k];
            continue;
        }
        if (hc[k] == 0.0) continue;
        double tmp = 0.0;
#pragma unroll
        for (int i = k + 1; i < N; ++i) tmp += A[i][k] * c[i];
        tmp += c[k];
        c[k] -= hc[k] * tmp;
#pragma unroll
        for (int i = k + 1; i < N; ++i) c[i] -= (hc[k] * A[i][k]) * tmp;
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        if (i < nonzero && c[i] != 0.0) {
            c[i] /= A[i][i];
#pragma unroll
            for (int j = 0; j < i; ++j) c[j] -= c[i] * A[j][i];
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
        if (i >= nonzero) c[i] = 0.0;
#pragma unroll
    for (int m = 0; m < N; ++m) {
        double v = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) v = (perm[i] == m) ? c[i] : v;
        xout[m] = v;
    }
}

}  // namespace lgs
