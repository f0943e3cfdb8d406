// What the projection code shares (projection_parse.hip fills it, proj_math.hpp and the kernels of projection.hip read it): a
// PROJ.4 string parsed into the constants of its closed forms.
#pragma once

#include "common.hpp"

namespace fimex_amd {

constexpr double kPi = 3.14159265358979323846;
constexpr double kHalfPi = kPi / 2, kFortPi = kPi / 4;
constexpr double kSpi = 3.14159265359;  // PROJ.4's adjlon threshold
constexpr double kEps10 = 1e-10;
constexpr double kDegToRad = .0174532925199432958;  // proj_api.h DEG_TO_RAD
constexpr double kRadToDeg = 57.29577951308232;     // proj_api.h RAD_TO_DEG

enum ProjKind { kLatLong = 0, kStere, kLcc, kMerc, kObTran, kTmerc, kEtmerc, kLaea, kAea, kGeos, kOmerc, kSinu, kCea, kOrtho, kAeqd, kNsper };
enum StereMode { kNorth = 0, kSouth, kOblique, kEquatorial };

// a kernel argument: layout and field order are part of the launch
struct ProjParams {
    int kind, mode, oblique, datum;
    double a, es, e, lam0, phi0, x0, y0, k0;
    double akm1, sinph0, cosph0;  // stere (on an ellipsoid: sin, cos of the conformal latitude of the origin)
    double n, c, rho0;            // lcc
    double lamp, sphip, cphip;    // ob_tran
    double esp, ml0, en[5];       // tmerc
    double Qn, Zb, cgb[6], cbg[6], utg[6], gtu[6];  // etmerc
    double qp, rq, dd, xmf, ymf, sinb1, cosb1, apa[3];  // laea (aea: dd, and n, c, rho0 of lcc)
    double ec, n2;                // aea
    double radius_g, radius_g_1, radius_p, radius_p2, radius_p_inv2, C;  // geos (flip_axis in mode)
    double pn1, pp, rp, pfact;    // nsper (sinph0 / cosph0 and the aspect in mode as for stere; sinu: en; cea: k0, qp, apa)
    double oA, oB, oE, ArB, BrA, rB, singam, cosgam, sinrot, cosrot, v_pole_n, v_pole_s, u_0;  // omerc (no_rot in mode)
    double towgs84[7];            // pj_datum_set: dx dy dz (m), rx ry rz (rad), scale factor
    double toMeter, frMeter;      // pj_init: +units / +to_meter (1 for metres); pj_fwd multiplies by fr_meter, pj_inv by to_meter
    double fromGreenwich;         // pj_init: +pm, radians east of Greenwich
    int datumType, doShift;       // 0 unknown, 1 three parameters, 2 seven, 3 WGS84; doShift: set on both sides of a pair that needs pj_datum_transform
};

// the two sides of one pj_transform; doShift is set when both name a datum and pj_compare_datums finds them different
struct ProjPair { ProjParams src, dst; };

// projection_parse.hip: throw Error with the reason for a string that is not supported; touch no device
ProjParams parse_proj4(const char* text);
ProjPair parse_pair(const char* projIn, const char* projOut);

}  // namespace fimex_amd
