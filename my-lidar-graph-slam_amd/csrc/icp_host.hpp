// icp_host.hpp -- the host-only code of the point-to-line ICP matcher
// (k_icp.hip): argument checks, the usable-beam count behind the table cap and
// the covariance of lgs_icp_summary.  Plain C++ (no HIP), so that
// tests/cpp_icp/icp_host_check.cpp runs it on its own under the sanitizers.
#pragma once

#include <cmath>

#include "lgs_hip.h"

namespace lgs {

constexpr int kIcpTableCap = 4096;   // usable reference beams: the table lives in LDS

inline bool icp_pose_finite(const lgs_pose2d& p)
{
    return std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.theta);
}

// LGS_OK or LGS_ERR_INVALID_ARG (the list of include/lgs_hip.h)
inline int icp_params_check(const lgs_icp_params* p)
{
    if (!p) return LGS_ERR_INVALID_ARG;
    const double v[7] = { p->convergence_threshold, p->usable_range_min, p->usable_range_max,
                          p->translation_regularizer, p->rotation_regularizer, p->max_correspondence_dist,
                          p->max_segment_length };
    for (double x : v)
        if (!std::isfinite(x)) return LGS_ERR_INVALID_ARG;
    if (p->max_correspondence_dist <= 0.0 || p->max_segment_length <= 0.0) return LGS_ERR_INVALID_ARG;
    if (p->translation_regularizer < 0.0 || p->rotation_regularizer < 0.0) return LGS_ERR_INVALID_ARG;
    return LGS_OK;
}

// a beam is usable iff !(r >= hi || r <= lo): the linear solver's comparisons
inline bool icp_usable(double r, double lo, double hi) { return !(r >= hi || r <= lo); }

inline int icp_usable_count(const double* ranges, int n, double lo, double hi)
{
    int m = 0;
    for (int j = 0; j < n; ++j) m += icp_usable(ranges[j], lo, hi) ? 1 : 0;
    return m;
}

// lgs_icp_summary::covariance (the header's comment, product by product)
inline void icp_covariance(const double H[9], double reg_t, double reg_r, double pair_cost, int num_pairs,
                           int pose_found, double cov[9])
{
    for (int k = 0; k < 9; ++k) cov[k] = 0.0;
    if (!pose_found) return;
    const double a0 = H[0] + reg_t, a1 = H[1], a2 = H[2];
    const double a3 = H[3], a4 = H[4] + reg_t, a5 = H[5];
    const double a6 = H[6], a7 = H[7], a8 = H[8] + reg_r;
    const double c[9] = { a4 * a8 - a5 * a7, a2 * a7 - a1 * a8, a1 * a5 - a2 * a4,
                          a5 * a6 - a3 * a8, a0 * a8 - a2 * a6, a2 * a3 - a0 * a5,
                          a3 * a7 - a4 * a6, a1 * a6 - a0 * a7, a0 * a4 - a1 * a3 };
    const double det = (a0 * c[0] + a1 * c[3]) + a2 * c[6];
    if (det == 0.0 || !std::isfinite(det)) return;
    const int dof = num_pairs - 3 > 1 ? num_pairs - 3 : 1;
    const double scale = pair_cost / (double)dof;
    for (int k = 0; k < 9; ++k) cov[k] = (c[k] / det) * scale;
}

}  // namespace lgs
