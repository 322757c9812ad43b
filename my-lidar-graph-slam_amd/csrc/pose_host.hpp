// pose_host.hpp -- the host pose algebra (glibc sincos, no contraction), free
// of the HIP runtime so that plain host programs can include it.
#pragma once

#include <cmath>

#include "lgs_hip.h"

extern "C" void sincos(double x, double* s, double* c);  // glibc

namespace lgs {

// The reference is built with GCC, which fuses sin(x) and cos(x) of the same
// argument into one glibc sincos() call; glibc's sincos differs from separate
// sin/cos in ~0.1% of inputs.  Every host recomputation that must be
// bit-exact therefore calls sincos() explicitly wherever the reference
// evaluates both (HitPoint, Compound, MoveBackward, ...).
inline void ref_sincos(double x, double& s, double& c) { ::sincos(x, &s, &c); }

// Host pose algebra restated from H/pose.hpp (glibc sincos, no contraction).
inline lgs_pose2d compound(lgs_pose2d s, lgs_pose2d d)
{
    double sinT, cosT;
    ref_sincos(s.theta, sinT, cosT);
    return { cosT * d.x - sinT * d.y + s.x, sinT * d.x + cosT * d.y + s.y, s.theta + d.theta };
}
inline lgs_pose2d move_backward(lgs_pose2d e, lgs_pose2d d)
{
    const double theta = e.theta - d.theta;
    double sinT, cosT;
    ref_sincos(theta, sinT, cosT);
    return { e.x - cosT * d.x + sinT * d.y, e.y - sinT * d.x - cosT * d.y, theta };
}
inline lgs_pose2d inverse_compound(lgs_pose2d s, lgs_pose2d e)
{
    double sinT, cosT;
    ref_sincos(s.theta, sinT, cosT);
    const double dx = e.x - s.x, dy = e.y - s.y;
    return { cosT * dx + sinT * dy, -sinT * dx + cosT * dy, e.theta - s.theta };
}
// NormalizeAngle (H/util.hpp:125-135): the C library's fmod, then one turn
inline double normalize_angle(double theta)
{
    const double pi = 3.14159265358979323846;   // M_PI
    double t = ::fmod(theta, 2.0 * pi);
    if (t > pi)
        t -= 2.0 * pi;
    else if (t < -pi)
        t += 2.0 * pi;
    return t;
}

}  // namespace lgs
