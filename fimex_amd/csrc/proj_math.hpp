// The point math of the coordinate transforms (pj_transform of PROJ.4 4.x on one point), for the kernels of projection.hip and,
// compiled for the host, for tests/projection_host.hip: one forward and one inverse function per projection, the datum shift,
// and the per-point parts of the rotation matrix and of the bounding-box reduction.
//
// PROJ.4 is a third-party library that is not part of the reference tree; the projections are implemented from their published
// closed forms (Snyder, "Map Projections - A Working Manual", USGS PP 1395) with PROJ.4's conventions at the pj_transform
// boundary: geographic coordinates in radians, projected x = a * x' + x_0, longitudes relative to lon_0 wrapped to [-pi, pi].
// On an ellipsoid the series are the ones PROJ.4 4.x uses (Snyder eq. 7-7, 7-9, 15-7..15-11, 21-33..21-40, 8-9..8-25, 3-21).
// A point a projection cannot map is NaN where pj_transform reports an error.
//
// Every operation keeps the order and type it has in PROJ.4 (the library is built with -ffp-contract=off).  Nothing here uses a
// device builtin; a forward / inverse function takes (lam, phi) relative to lon_0 on the unit sphere or ellipsoid and gives the
// unscaled (x', y'), or the other way round.  What the projections share around that is in proj_forward / proj_inverse.
#pragma once

#include "proj_params.hpp"

#include <cmath>

#define FA_HD __host__ __device__ __forceinline__

namespace fimex_amd {

// pj_tsfn / pj_msfn / pj_qsfn (Snyder eq. 3-12) / ssfn_ of PJ_stere.c / pj_phi2 / pj_mlfn / pj_inv_mlfn
FA_HD double tsfn(double phi, double sinphi, double e)
{
    sinphi *= e;
    return tan(.5 * (kHalfPi - phi)) / pow((1. - sinphi) / (1. + sinphi), .5 * e);
}
FA_HD double msfn(double sinphi, double cosphi, double es) { return cosphi / sqrt(1. - es * sinphi * sinphi); }
FA_HD double qsfn(double sinphi, double e, double one_es)
{
    if (e >= 1e-7) {
        const double con = e * sinphi;
        return one_es * (sinphi / (1. - con * con) - (.5 / e) * log((1. - con) / (1. + con)));
    }
    return sinphi + sinphi;
}
FA_HD double ssfn(double phit, double sinphi, double e)
{
    sinphi *= e;
    return tan(.5 * (kHalfPi + phit)) * pow((1. - sinphi) / (1. + sinphi), .5 * e);
}
FA_HD double phi2(double ts, double e)
{
    const double eccnth = .5 * e;
    double phi = kHalfPi - 2. * atan(ts), dphi;
    int i = 15;
    do {
        const double con = e * sin(phi);
        dphi = kHalfPi - 2. * atan(ts * pow((1. - con) / (1. + con), eccnth)) - phi;
        phi += dphi;
    } while (fabs(dphi) > 1e-10 && --i);
    return i ? phi : NAN;  // pj_phi2 reports an error after 15 rounds
}
FA_HD double mlfn(double phi, double sphi, double cphi, const double* en)
{
    cphi *= sphi;
    sphi *= sphi;
    return en[0] * phi - cphi * (en[1] + sphi * (en[2] + sphi * (en[3] + sphi * en[4])));
}
FA_HD double inv_mlfn(double arg, double es, const double* en)
{
    const double k = 1. / (1. - es);
    double phi = arg;
    for (int i = 10; i; --i) {
        const double s = sin(phi);
        double t = 1. - es * s * s;
        phi -= t = (mlfn(phi, s, cos(phi), en) - arg) * (t * sqrt(t)) * k;
        if (fabs(t) < 1e-11) return phi;
    }
    return NAN;
}
// pj_authlat: the geodetic latitude of an authalic one
FA_HD double authlat(double beta, const double* apa)
{
    const double t = beta + beta;
    return beta + apa[0] * sin(t) + apa[1] * sin(t + t) + apa[2] * sin(t + t + t);
}

// PJ_etmerc.c: Clenshaw summation of sum p[k] sin(2 (k+1) B) + B, and of the complex sine series
FA_HD double gatg(const double* p1, double B)
{
    const double cos2B = 2 * cos(2 * B);
    double h = 0, h1 = p1[5], h2 = 0;
    for (int k = 4; k >= 0; --k) {
        h = -h2 + cos2B * h1 + p1[k];
        h2 = h1;
        h1 = h;
    }
    return B + h * sin(2 * B);
}
FA_HD void clenS(const double* a, double argR, double argI, double& R, double& I)
{
    const double sinR = sin(argR), cosR = cos(argR), sinhI = sinh(argI), coshI = cosh(argI);
    double r = 2 * cosR * coshI, i = -2 * sinR * sinhI;
    double hr = a[5], hi = 0, hr1 = 0, hi1 = 0, hr2, hi2;
    for (int k = 4; k >= 0; --k) {
        hr2 = hr1;
        hi2 = hi1;
        hr1 = hr;
        hi1 = hi;
        hr = -hr2 + r * hr1 - i * hi1 + a[k];
        hi = -hi2 + i * hr1 + r * hi1;
    }
    r = sinR * coshI;
    i = cosR * sinhI;
    R = r * hr - i * hi;
    I = r * hi + i * hr;
}

FA_HD double adjlon(double lon)
{
    if (fabs(lon) <= kSpi) return lon;
    lon += kPi;
    lon -= 2 * kPi * floor(lon / (2 * kPi));
    return lon - kPi;
}

// ---- stere: PJ_stere.c e_forward / s_forward, e_inverse / s_inverse ----
FA_HD void stere_forward(const ProjParams& p, double lam, double phi, double& px, double& py)
{
    const double sinlam = sin(lam);
    double coslam = cos(lam);
    if (p.es != 0) {
        double sinphi = sin(phi);
        if (p.mode == kOblique) {
            const double X = 2. * atan(ssfn(phi, sinphi, p.e)) - kHalfPi;
            const double sinX = sin(X), cosX = cos(X);
            const double A = p.akm1 / (p.cosph0 * (1. + p.sinph0 * sinX + p.cosph0 * cosX * coslam));
            py = A * (p.cosph0 * sinX - p.sinph0 * cosX * coslam);
            px = A * cosX;
        } else {
            if (p.mode == kSouth) { phi = -phi; coslam = -coslam; sinphi = -sinphi; }
            px = p.akm1 * tsfn(phi, sinphi, p.e);
            py = -px * coslam;
        }
        px *= sinlam;
    } else if (p.mode == kNorth || p.mode == kSouth) {
        if (p.mode == kNorth) { coslam = -coslam; phi = -phi; }
        py = p.akm1 * tan(kFortPi + .5 * phi);
        px = sinlam * py;
        py *= coslam;
    } else {
        const double sinphi = sin(phi), cosphi = cos(phi);
        if (p.mode == kEquatorial) {
            const double k = p.akm1 / (1. + cosphi * coslam);
            px = k * cosphi * sinlam;
            py = k * sinphi;
        } else {
            const double k = p.akm1 / (1. + p.sinph0 * sinphi + p.cosph0 * cosphi * coslam);
            px = k * cosphi * sinlam;
            py = k * (p.cosph0 * sinphi - p.sinph0 * cosphi * coslam);
        }
    }
}
FA_HD void stere_inverse(const ProjParams& p, double xs, double ys, double& lam, double& phi)
{
    if (p.es != 0) {
        const double rho = hypot(xs, ys);
        double tp, phi_l, halfpi, halfe;
        if (p.mode == kOblique) {
            tp = 2. * atan2(rho * p.cosph0, p.akm1);
            const double cosphi = cos(tp), sinphi = sin(tp);
            phi_l = rho == 0. ? asin(cosphi * p.sinph0) : asin(cosphi * p.sinph0 + (ys * sinphi * p.cosph0 / rho));
            tp = tan(.5 * (kHalfPi + phi_l));
            xs *= sinphi;
            ys = rho * p.cosph0 * cosphi - ys * p.sinph0 * sinphi;
            halfpi = kHalfPi;
            halfe = .5 * p.e;
        } else {
            if (p.mode == kNorth) ys = -ys;
            phi_l = kHalfPi - 2. * atan(tp = -rho / p.akm1);
            halfpi = -kHalfPi;
            halfe = -.5 * p.e;
        }
        phi = NAN;  // no convergence in 8 rounds: pj_transform reports an error
        lam = NAN;
        for (int i = 8; i--; phi_l = phi) {
            const double sinphi = p.e * sin(phi_l);
            phi = 2. * atan(tp * pow((1. + sinphi) / (1. - sinphi), halfe)) - halfpi;
            if (fabs(phi_l - phi) < 1e-10) {
                if (p.mode == kSouth) phi = -phi;
                lam = (xs == 0. && ys == 0.) ? 0. : atan2(xs, ys);
                break;
            }
            if (i == 0) phi = NAN;
        }
        return;
    }
    const double rh = hypot(xs, ys);
    const double c = 2. * atan(rh / p.akm1);
    const double sinc = sin(c), cosc = cos(c);
    if (p.mode == kNorth) {
        ys = -ys;
        phi = (fabs(rh) <= kEps10) ? p.phi0 : asin(cosc);
        lam = (xs == 0. && ys == 0.) ? 0. : atan2(xs, ys);
    } else if (p.mode == kSouth) {
        phi = (fabs(rh) <= kEps10) ? p.phi0 : asin(-cosc);
        lam = (xs == 0. && ys == 0.) ? 0. : atan2(xs, ys);
    } else if (p.mode == kEquatorial) {
        phi = (fabs(rh) <= kEps10) ? 0. : asin(ys * sinc / rh);
        lam = (cosc != 0. || xs != 0.) ? atan2(xs * sinc, cosc * rh) : 0.;
    } else {
        phi = (fabs(rh) <= kEps10) ? p.phi0 : asin(cosc * p.sinph0 + ys * sinc * p.cosph0 / rh);
        const double cc = cosc - p.sinph0 * sin(phi);
        lam = (cc != 0. || xs != 0.) ? atan2(xs * sinc * p.cosph0, cc * rh) : 0.;
    }
}

// ---- lcc: PJ_lcc.c ----
FA_HD void lcc_forward(const ProjParams& p, double lam, double phi, double& px, double& py)
{
    const double rho = (fabs(fabs(phi) - kHalfPi) < kEps10) ? 0.
                       : p.c * (p.es != 0 ? pow(tsfn(phi, sin(phi), p.e), p.n) : pow(tan(kFortPi + .5 * phi), -p.n));
    lam *= p.n;
    px = p.k0 * (rho * sin(lam));
    py = p.k0 * (p.rho0 - rho * cos(lam));
}
FA_HD void lcc_inverse(const ProjParams& p, double xs, double ys, double& lam, double& phi)
{
    xs /= p.k0;
    ys = p.rho0 - ys / p.k0;
    double rho = hypot(xs, ys);
    if (rho != 0.) {
        if (p.n < 0.) { rho = -rho; xs = -xs; ys = -ys; }
        phi = p.es != 0 ? phi2(pow(rho / p.c, 1. / p.n), p.e) : 2. * atan(pow(p.c / rho, 1. / p.n)) - kHalfPi;
        lam = atan2(xs, ys) / p.n;
    } else {
        lam = 0.;
        phi = p.n > 0. ? kHalfPi : -kHalfPi;
    }
}

// ---- merc: PJ_merc.c ----
FA_HD void merc_forward(const ProjParams& p, double lam, double phi, double& px, double& py)
{
    px = p.k0 * lam;
    py = p.es != 0 ? -p.k0 * log(tsfn(phi, sin(phi), p.e)) : p.k0 * log(tan(kFortPi + .5 * phi));
}
FA_HD void merc_inverse(const ProjParams& p, double xs, double ys, double& lam, double& phi)
{
    lam = xs / p.k0;
    phi = p.es != 0 ? phi2(exp(-ys / p.k0), p.e) : kHalfPi - 2. * atan(exp(-ys / p.k0));
}

// ---- tmerc: PJ_tmerc.c (4.x), the Gauss-Krueger series on the ellipsoid, the closed form on the sphere ----
constexpr double FC1 = 1., FC2 = .5, FC3 = .16666666666666666666, FC4 = .08333333333333333333, FC5 = .05,
                 FC6 = .03333333333333333333, FC7 = .02380952380952380952, FC8 = .01785714285714285714;
FA_HD void tmerc_forward(const ProjParams& p, double lam, double phi, double& px, double& py)
{
    const double sinphi = sin(phi), cosphi = cos(phi);
    if (p.es != 0) {
        if (lam < -kHalfPi || lam > kHalfPi) { px = NAN; py = NAN; }
        else {
            double t = fabs(cosphi) > 1e-10 ? sinphi / cosphi : 0.;
            t *= t;
            double al = cosphi * lam;
            const double als = al * al;
            al /= sqrt(1. - p.es * sinphi * sinphi);
            const double n = p.esp * cosphi * cosphi;
            px = p.k0 * al * (FC1 + FC3 * als * (1. - t + n + FC5 * als * (5. + t * (t - 18.) + n * (14. - 58. * t) +
                              FC7 * als * (61. + t * (t * (179. - t) - 479.)))));
            py = p.k0 * (mlfn(phi, sinphi, cosphi, p.en) - p.ml0 + sinphi * al * lam * FC2 * (1. + FC4 * als * (5. - t + n * (9. + 4. * n) +
                         FC6 * als * (61. + t * (t - 58.) + n * (270. - 330. * t) + FC8 * als * (1385. + t * (t * (543. - t) - 3111.))))));
        }
    } else {
        double b = cosphi * sin(lam);
        if (fabs(fabs(b) - 1.) <= kEps10) { px = NAN; py = NAN; }
        else {
            px = p.ml0 * log((1. + b) / (1. - b));
            py = cosphi * cos(lam) / sqrt(1. - b * b);
            b = fabs(py);
            py = b >= 1. ? 0. : acos(py);
            if (phi < 0.) py = -py;
            py = p.esp * (py - p.phi0);
        }
    }
}
FA_HD void tmerc_inverse(const ProjParams& p, double xs, double ys, double& lam, double& phi)
{
    if (p.es != 0) {
        phi = inv_mlfn(p.ml0 + ys / p.k0, p.es, p.en);
        if (fabs(phi) >= kHalfPi) {
            phi = ys < 0. ? -kHalfPi : kHalfPi;
            lam = 0.;
        } else {
            const double sinphi = sin(phi), cosphi = cos(phi);
            double t = fabs(cosphi) > 1e-10 ? sinphi / cosphi : 0.;
            const double n = p.esp * cosphi * cosphi;
            double con = 1. - p.es * sinphi * sinphi;
            const double d = xs * sqrt(con) / p.k0;
            con *= t;
            t *= t;
            const double ds = d * d;
            phi -= (con * ds / (1. - p.es)) * FC2 * (1. - ds * FC4 * (5. + t * (3. - 9. * n) + n * (1. - 4 * n) -
                    ds * FC6 * (61. + t * (90. - 252. * n + 45. * t) + 46. * n - ds * FC8 * (1385. + t * (3633. + t * (4095. + 1574. * t))))));
            lam = d * (FC1 - ds * FC3 * (1. + 2. * t + n - ds * FC5 * (5. + t * (28. + 24. * t + 8. * n) + 6. * n -
                       ds * FC7 * (61. + t * (662. + t * (1320. + 720. * t)))))) / cosphi;
        }
    } else {
        double h = exp(xs / p.esp);
        const double g = .5 * (h - 1. / h);
        h = cos(p.phi0 + ys / p.esp);
        phi = asin(sqrt((1. - h * h) / (1. + g * g)));
        if (ys < 0. && -phi + p.phi0 < 0.) phi = -phi;  // the hemisphere test of PROJ 4.9 (4.8 and older: y < 0 alone, wrong for lat_0 != 0)
        lam = (g != 0. || h != 0.) ? atan2(g, h) : 0.;
    }
}

// ---- sinu: PJ_gn_sinu.c ----
FA_HD void sinu_forward(const ProjParams& p, double lam, double phi, double& px, double& py)
{
    const double sn = sin(phi), cs = cos(phi);
    if (p.es != 0) { py = mlfn(phi, sn, cs, p.en); px = lam * cs / sqrt(1. - p.es * sn * sn); }
    else { px = lam * cs; py = phi; }
}
FA_HD void sinu_inverse(const ProjParams& p, double xs, double ys, double& lam, double& phi)
{
    if (p.es != 0) {
        phi = inv_mlfn(ys, p.es, p.en);
        const double ab = fabs(phi);
        if (ab < kHalfPi) {
            const double sn = sin(phi);
            lam = xs * sqrt(1. - p.es * sn * sn) / cos(phi);
        } else if (ab - kEps10 < kHalfPi) lam = 0.;
        else { lam = NAN; phi = NAN; }
    } else {
        phi = ys;
        lam = xs / cos(ys);
    }
}

// ---- cea: PJ_cea.c ----
FA_HD void cea_forward(const ProjParams& p, double lam, double phi, double& px, double& py)
{
    px = p.k0 * lam;
    py = p.es != 0 ? .5 * qsfn(sin(phi), p.e, 1. - p.es) / p.k0 : sin(phi) / p.k0;
}
FA_HD void cea_inverse(const ProjParams& p, double xs, double ys, double& lam, double& phi)
{
    lam = xs / p.k0;
    if (p.es != 0) {
        double q = 2. * ys * p.k0 / p.qp;
        q = q > 1 ? 1 : (q < -1 ? -1 : q);
        phi = authlat(asin(q), p.apa);
    } else {
        ys *= p.k0;
        const double t = fabs(ys);
        if (t - kEps10 <= 1.) phi = t >= 1. ? (ys < 0. ? -kHalfPi : kHalfPi) : asin(ys);
        else { phi = NAN; lam = NAN; }
    }
}

// ---- ortho: PJ_ortho.c, sphere ----
FA_HD void ortho_forward(const ProjParams& p, double lam, double phi, double& px, double& py)
{
    const double cosphi = cos(phi), sinphi = sin(phi);
    double coslam = cos(lam);
    bool bad;
    if (p.mode == kEquatorial) { bad = cosphi * coslam < -kEps10; py = sinphi; }
    else if (p.mode == kOblique) {
        bad = p.sinph0 * sinphi + p.cosph0 * cosphi * coslam < -kEps10;
        py = p.cosph0 * sinphi - p.sinph0 * cosphi * coslam;
    } else {
        if (p.mode == kNorth) coslam = -coslam;
        bad = fabs(phi - p.phi0) - kEps10 > kHalfPi;
        py = cosphi * coslam;
    }
    px = cosphi * sin(lam);
    if (bad) { px = NAN; py = NAN; }
}
FA_HD void ortho_inverse(const ProjParams& p, double xs, double ys, double& lam, double& phi)
{
    const double rh = hypot(xs, ys);
    double sinc = rh;
    if (sinc - 1. > kEps10) { phi = NAN; lam = NAN; return; }
    if (sinc > 1.) sinc = 1.;
    const double cosc = sqrt(1. - sinc * sinc);
    if (fabs(rh) <= kEps10) { phi = p.phi0; lam = 0.; return; }
    if (p.mode == kNorth) { ys = -ys; phi = acos(sinc); }
    else if (p.mode == kSouth) phi = -acos(sinc);
    else {
        if (p.mode == kEquatorial) { phi = ys * sinc / rh; xs *= sinc; ys = cosc * rh; }
        else {
            phi = cosc * p.sinph0 + ys * sinc * p.cosph0 / rh;
            ys = (cosc - p.sinph0 * phi) * rh;
            xs *= sinc * p.cosph0;
        }
        phi = fabs(phi) >= 1. ? (phi < 0. ? -kHalfPi : kHalfPi) : asin(phi);
    }
    lam = (ys == 0. && (p.mode == kOblique || p.mode == kEquatorial)) ? (xs == 0. ? 0. : (xs < 0. ? -kHalfPi : kHalfPi)) : atan2(xs, ys);
}

// ---- aeqd: PJ_aeqd.c, sphere ----
FA_HD void aeqd_forward(const ProjParams& p, double lam, double phi, double& px, double& py)
{
    const double sinphi = sin(phi), cosphi = cos(phi);
    double coslam = cos(lam);
    if (p.mode == kEquatorial || p.mode == kOblique) {
        py = p.mode == kEquatorial ? cosphi * coslam : p.sinph0 * sinphi + p.cosph0 * cosphi * coslam;
        if (fabs(fabs(py) - 1.) < 1e-14) {
            if (py < 0.) { px = NAN; py = NAN; }
            else { px = 0.; py = 0.; }
        } else {
            py = acos(py);
            py /= sin(py);
            px = py * cosphi * sin(lam);
            py *= p.mode == kEquatorial ? sinphi : p.cosph0 * sinphi - p.sinph0 * cosphi * coslam;
        }
    } else {
        if (p.mode == kNorth) { phi = -phi; coslam = -coslam; }
        if (fabs(phi - kHalfPi) < kEps10) { px = NAN; py = NAN; }
        else {
            py = kHalfPi + phi;
            px = py * sin(lam);
            py *= coslam;
        }
    }
}
FA_HD void aeqd_inverse(const ProjParams& p, double xs, double ys, double& lam, double& phi)
{
    double c_rh = hypot(xs, ys);
    if (c_rh - kEps10 > kPi) { phi = NAN; lam = NAN; }
    else if (c_rh < kEps10) { phi = p.phi0; lam = 0.; }
    else {
        if (c_rh > kPi) c_rh = kPi;
        if (p.mode == kOblique || p.mode == kEquatorial) {
            const double sinc = sin(c_rh), cosc = cos(c_rh);
            double arg;
            if (p.mode == kEquatorial) { arg = ys * sinc / c_rh; xs *= sinc; ys = cosc * c_rh; }
            else {
                arg = cosc * p.sinph0 + ys * sinc * p.cosph0 / c_rh;
                arg = arg > 1 ? 1 : (arg < -1 ? -1 : arg);
                ys = (cosc - p.sinph0 * arg) * c_rh;  // sin(asin(arg))
                xs *= sinc * p.cosph0;
            }
            arg = arg > 1 ? 1 : (arg < -1 ? -1 : arg);
            phi = asin(arg);
            lam = ys == 0. ? 0. : atan2(xs, ys);
        } else if (p.mode == kNorth) { phi = kHalfPi - c_rh; lam = atan2(xs, -ys); }
        else { phi = c_rh - kHalfPi; lam = atan2(xs, ys); }
    }
}

// ---- nsper: PJ_nsper.c, sphere, no tilt ----
FA_HD void nsper_forward(const ProjParams& p, double lam, double phi, double& px, double& py)
{
    const double sinphi = sin(phi), cosphi = cos(phi), coslam = cos(lam);
    py = p.mode == kOblique ? p.sinph0 * sinphi + p.cosph0 * cosphi * coslam
         : (p.mode == kEquatorial ? cosphi * coslam : (p.mode == kSouth ? -sinphi : sinphi));
    if (py < p.rp) { px = NAN; py = NAN; }  // beyond the horizon
    else {
        py = p.pn1 / (p.pp - py);
        px = py * cosphi * sin(lam);
        if (p.mode == kOblique) py *= p.cosph0 * sinphi - p.sinph0 * cosphi * coslam;
        else if (p.mode == kEquatorial) py *= sinphi;
        else py *= cosphi * (p.mode == kNorth ? -coslam : coslam);
    }
}
FA_HD void nsper_inverse(const ProjParams& p, double xs, double ys, double& lam, double& phi)
{
    const double rh = hypot(xs, ys);
    double sinz = 1. - rh * rh * p.pfact;
    if (sinz < 0.) { phi = NAN; lam = NAN; }
    else if (fabs(rh) <= kEps10) { lam = 0.; phi = p.phi0; }
    else {
        sinz = (p.pp - sqrt(sinz)) / (p.pn1 / rh + rh / p.pn1);
        const double cosz = sqrt(1. - sinz * sinz);
        if (p.mode == kOblique) {
            phi = asin(cosz * p.sinph0 + ys * sinz * p.cosph0 / rh);
            ys = (cosz - p.sinph0 * sin(phi)) * rh;
            xs *= sinz * p.cosph0;
        } else if (p.mode == kEquatorial) {
            phi = asin(ys * sinz / rh);
            ys = cosz * rh;
            xs *= sinz;
        } else if (p.mode == kNorth) { phi = asin(cosz); ys = -ys; }
        else phi = -asin(cosz);
        lam = atan2(xs, ys);
    }
}

// ---- omerc: PJ_omerc.c ----
FA_HD void omerc_forward(const ProjParams& p, double lam, double phi, double& px, double& py)
{
    double u, v;
    bool ok = true;
    if (fabs(fabs(phi) - kHalfPi) > kEps10) {
        const double Q = p.oE / pow(tsfn(phi, sin(phi), p.e), p.oB);
        const double temp = 1. / Q, S = .5 * (Q - temp), T = .5 * (Q + temp);
        const double V = sin(p.oB * lam), U = (S * p.singam - V * p.cosgam) / T;
        if (fabs(fabs(U) - 1.0) < kEps10) ok = false;
        v = 0.5 * p.ArB * log((1. - U) / (1. + U));
        u = p.ArB * atan2((S * p.cosgam + V * p.singam), cos(p.oB * lam));
    } else {
        v = phi > 0 ? p.v_pole_n : p.v_pole_s;
        u = p.ArB * phi;
    }
    if (!ok) { px = NAN; py = NAN; }
    else if (p.mode) { px = u; py = v; }
    else {
        u -= p.u_0;
        px = v * p.cosrot + u * p.sinrot;
        py = u * p.cosrot - v * p.sinrot;
    }
}
FA_HD void omerc_inverse(const ProjParams& p, double xs, double ys, double& lam, double& phi)
{
    double u, v;
    if (p.mode) { v = ys; u = xs; }
    else {
        v = xs * p.cosrot - ys * p.sinrot;
        u = ys * p.cosrot + xs * p.sinrot + p.u_0;
    }
    const double Qp = exp(-p.BrA * v), Sp = .5 * (Qp - 1. / Qp), Tp = .5 * (Qp + 1. / Qp);
    const double Vp = sin(p.BrA * u), Up = (Vp * p.cosgam + Sp * p.singam) / Tp;
    if (fabs(fabs(Up) - 1.) < kEps10) {
        lam = 0.;
        phi = Up < 0. ? -kHalfPi : kHalfPi;
    } else {
        phi = p.oE / sqrt((1. + Up) / (1. - Up));
        phi = phi2(pow(phi, 1. / p.oB), p.e);
        lam = -p.rB * atan2((Sp * p.cosgam - Vp * p.singam), cos(p.BrA * u));
    }
}

// ---- geos: PJ_geos.c e_forward / e_inverse (the spherical form is this one with radius_p = 1) ----
FA_HD void geos_forward(const ProjParams& p, double lam, double phi, double& px, double& py)
{
    phi = atan(p.radius_p2 * tan(phi));
    const double r = p.radius_p / hypot(p.radius_p * cos(phi), sin(phi));
    const double Vx = r * cos(lam) * cos(phi), Vy = r * sin(lam) * cos(phi), Vz = r * sin(phi);
    if (((p.radius_g - Vx) * Vx - Vy * Vy - Vz * Vz * p.radius_p_inv2) < 0.) { px = NAN; py = NAN; }  // behind the limb
    else {
        const double tmp = p.radius_g - Vx;
        if (p.mode) { px = p.radius_g_1 * atan(Vy / hypot(Vz, tmp)); py = p.radius_g_1 * atan(Vz / tmp); }
        else { px = p.radius_g_1 * atan(Vy / tmp); py = p.radius_g_1 * atan(Vz / hypot(Vy, tmp)); }
    }
}
FA_HD void geos_inverse(const ProjParams& p, double xs, double ys, double& lam, double& phi)
{
    double Vx = -1.0, Vy, Vz;
    if (p.mode) { Vz = tan(ys / p.radius_g_1); Vy = tan(xs / p.radius_g_1) * hypot(1.0, Vz); }
    else { Vy = tan(xs / p.radius_g_1); Vz = tan(ys / p.radius_g_1) * hypot(1.0, Vy); }
    double a = Vz / p.radius_p;
    a = Vy * Vy + a * a + Vx * Vx;
    const double b = 2 * p.radius_g * Vx;
    const double det = (b * b) - 4 * a * p.C;
    if (det < 0.) { lam = NAN; phi = NAN; }  // off the disc
    else {
        const double k = (-b - sqrt(det)) / (2. * a);
        Vx = p.radius_g + k * Vx;
        Vy *= k;
        Vz *= k;
        lam = atan2(Vy, Vx);
        phi = atan(Vz * cos(lam) / Vx);
        phi = atan(p.radius_p_inv2 * tan(phi));
    }
}

// ---- aea: PJ_aea.c ----
FA_HD void aea_forward(const ProjParams& p, double lam, double phi, double& px, double& py)
{
    double rho = p.c - (p.es != 0 ? p.n * qsfn(sin(phi), p.e, 1. - p.es) : p.n2 * sin(phi));
    if (rho < 0.) { px = NAN; py = NAN; }
    else {
        rho = p.dd * sqrt(rho);
        lam *= p.n;
        px = rho * sin(lam);
        py = p.rho0 - rho * cos(lam);
    }
}
// pj_phi1_ of PJ_aea.c: Newton on the authalic q
FA_HD double aea_phi1(double qs, double e, double one_es)
{
    double Phi = asin(.5 * qs), dphi;
    int i = 15;
    do {
        const double sinpi = sin(Phi), cospi = cos(Phi), con = e * sinpi, com = 1. - con * con;
        dphi = .5 * com * com / cospi * (qs / one_es - sinpi / com + .5 / e * log((1. - con) / (1. + con)));
        Phi += dphi;
    } while (fabs(dphi) > 1e-10 && --i);
    return i ? Phi : NAN;
}
FA_HD void aea_inverse(const ProjParams& p, double xs, double ys, double& lam, double& phi)
{
    ys = p.rho0 - ys;
    double rho = hypot(xs, ys);
    if (rho != 0.) {
        if (p.n < 0.) { rho = -rho; xs = -xs; ys = -ys; }
        phi = rho / p.dd;
        if (p.es != 0) {
            phi = (p.c - phi * phi) / p.n;
            if (fabs(p.ec - fabs(phi)) > 1e-7) phi = aea_phi1(phi, p.e, 1. - p.es);
            else phi = phi < 0. ? -kHalfPi : kHalfPi;
        } else {
            phi = (p.c - phi * phi) / p.n2;
            phi = fabs(phi) <= 1. ? asin(phi) : (phi < 0. ? -kHalfPi : kHalfPi);
        }
        lam = atan2(xs, ys) / p.n;
    } else {
        lam = 0.;
        phi = p.n > 0. ? kHalfPi : -kHalfPi;
    }
}

// ---- laea: PJ_laea.c e_forward / s_forward, e_inverse / s_inverse ----
FA_HD void laea_forward(const ProjParams& p, double lam, double phi, double& px, double& py)
{
    double coslam = cos(lam);
    const double sinlam = sin(lam), sinphi = sin(phi);
    if (p.es != 0) {
        double q = qsfn(sinphi, p.e, 1. - p.es), b;
        if (p.mode == kOblique || p.mode == kEquatorial) {
            const double sinb = q / p.qp, cosb = sqrt(1. - sinb * sinb);
            if (p.mode == kOblique) {
                b = 1. + p.sinb1 * sinb + p.cosb1 * cosb * coslam;
                if (fabs(b) < kEps10) { px = NAN; py = NAN; }
                else {
                    b = sqrt(2. / b);
                    py = p.ymf * b * (p.cosb1 * sinb - p.sinb1 * cosb * coslam);
                    px = p.xmf * b * cosb * sinlam;
                }
            } else {
                b = 1. + cosb * coslam;
                if (fabs(b) < kEps10) { px = NAN; py = NAN; }
                else {
                    b = sqrt(2. / b);
                    py = b * sinb * p.ymf;
                    px = p.xmf * b * cosb * sinlam;
                }
            }
        } else {
            if (p.mode == kNorth) { b = kHalfPi + phi; q = p.qp - q; }
            else { b = phi - kHalfPi; q = p.qp + q; }
            if (fabs(b) < kEps10) { px = NAN; py = NAN; }
            else if (q >= 0.) {
                b = sqrt(q);
                px = b * sinlam;
                py = coslam * (p.mode == kSouth ? b : -b);
            } else { px = 0.; py = 0.; }
        }
    } else {
        const double cosphi = cos(phi);
        if (p.mode == kEquatorial || p.mode == kOblique) {
            py = p.mode == kEquatorial ? 1. + cosphi * coslam : 1. + p.sinb1 * sinphi + p.cosb1 * cosphi * coslam;
            if (py <= kEps10) { px = NAN; py = NAN; }
            else {
                py = sqrt(2. / py);
                px = py * cosphi * sinlam;
                py *= p.mode == kEquatorial ? sinphi : p.cosb1 * sinphi - p.sinb1 * cosphi * coslam;
            }
        } else {
            if (p.mode == kNorth) coslam = -coslam;
            if (fabs(phi + p.phi0) < kEps10) { px = NAN; py = NAN; }
            else {
                py = kFortPi - phi * .5;
                py = 2. * (p.mode == kSouth ? cos(py) : sin(py));
                px = py * sinlam;
                py *= coslam;
            }
        }
    }
}
FA_HD void laea_inverse(const ProjParams& p, double xs, double ys, double& lam, double& phi)
{
    if (p.es != 0) {
        double ab = 0;
        bool centre = false;
        if (p.mode == kEquatorial || p.mode == kOblique) {
            xs /= p.dd;
            ys *= p.dd;
            const double rho = hypot(xs, ys);
            if (rho < kEps10) centre = true;
            else {
                double sCe = 2. * asin(.5 * rho / p.rq);
                const double cCe = cos(sCe);
                sCe = sin(sCe);
                xs *= sCe;
                if (p.mode == kOblique) {
                    ab = cCe * p.sinb1 + ys * sCe * p.cosb1 / rho;
                    ys = rho * p.cosb1 * cCe - ys * p.sinb1 * sCe;
                } else {
                    ab = ys * sCe / rho;
                    ys = rho * cCe;
                }
            }
        } else {
            if (p.mode == kNorth) ys = -ys;
            const double q = xs * xs + ys * ys;
            if (q == 0.) centre = true;
            else {
                ab = 1. - q / p.qp;
                if (p.mode == kSouth) ab = -ab;
            }
        }
        if (centre) { lam = 0.; phi = p.phi0; }
        else {
            lam = atan2(xs, ys);
            phi = authlat(asin(ab), p.apa);
        }
    } else {
        const double rh = hypot(xs, ys);
        phi = rh * .5;
        if (phi > 1.) { phi = NAN; lam = NAN; }
        else {
            phi = 2. * asin(phi);
            const double sinz = sin(phi), cosz = cos(phi);
            if (p.mode == kEquatorial) {
                phi = fabs(rh) <= kEps10 ? 0. : asin(ys * sinz / rh);
                xs *= sinz;
                ys = cosz * rh;
            } else if (p.mode == kOblique) {
                phi = fabs(rh) <= kEps10 ? p.phi0 : asin(cosz * p.sinb1 + ys * sinz * p.cosb1 / rh);
                xs *= sinz * p.cosb1;
                ys = (cosz - sin(phi) * p.sinb1) * rh;
            } else if (p.mode == kNorth) {
                ys = -ys;
                phi = kHalfPi - phi;
            } else {
                phi -= kHalfPi;
            }
            lam = (ys == 0. && (p.mode == kEquatorial || p.mode == kOblique)) ? 0. : atan2(xs, ys);
        }
    }
}

// ---- etmerc (and utm): PJ_etmerc.c ----
FA_HD void etmerc_forward(const ProjParams& p, double lam, double phi, double& px, double& py)
{
    double Cn = gatg(p.cbg, phi), Ce = lam;                     // geodetic -> Gaussian latitude
    const double sinCn = sin(Cn), cosCn = cos(Cn), sinCe = sin(Ce), cosCe = cos(Ce);
    Cn = atan2(sinCn, cosCe * cosCn);                           // -> complementary spherical
    Ce = atan2(sinCe * cosCn, hypot(sinCn, cosCn * cosCe));
    Ce = asinh(tan(Ce));
    double dCn, dCe;
    clenS(p.gtu, 2 * Cn, 2 * Ce, dCn, dCe);                     // -> normalised ellipsoidal N, E
    Cn += dCn;
    Ce += dCe;
    if (fabs(Ce) <= 2.623395162778) { py = p.Qn * Cn + p.Zb; px = p.Qn * Ce; }
    else { px = NAN; py = NAN; }
}
FA_HD void etmerc_inverse(const ProjParams& p, double xs, double ys, double& lam, double& phi)
{
    double Cn = (ys - p.Zb) / p.Qn, Ce = xs / p.Qn;
    if (fabs(Ce) <= 2.623395162778) {
        double dCn, dCe;
        clenS(p.utg, 2 * Cn, 2 * Ce, dCn, dCe);
        Cn += dCn;
        Ce += dCe;
        Ce = atan(sinh(Ce));
        const double sinCn = sin(Cn), cosCn = cos(Cn), sinCe = sin(Ce), cosCe = cos(Ce);
        Ce = atan2(sinCe, cosCe * cosCn);
        Cn = atan2(sinCn * cosCe, hypot(sinCe, cosCe * cosCn));
        phi = gatg(p.cgb, Cn);
        lam = Ce;
    } else { phi = NAN; lam = NAN; }
}

// ---- ob_tran + o_proj=longlat: PJ_ob_tran.c; radians stay radians, and px already holds the rotated longitude ----
FA_HD void ob_tran_forward(const ProjParams& p, double lam, double phi, double& px, double& py)
{
    if (p.oblique) {
        const double coslam = cos(lam), sinphi = sin(phi), cosphi = cos(phi);
        px = adjlon(atan2(cosphi * sin(lam), p.sphip * cosphi * coslam + p.cphip * sinphi) + p.lamp);
        double s = p.sphip * sinphi - p.cphip * cosphi * coslam;
        s = s > 1 ? 1 : (s < -1 ? -1 : s);
        py = asin(s);
    } else {
        px = adjlon(lam + p.lamp);
        py = phi;
    }
}
FA_HD void ob_tran_inverse(const ProjParams& p, double xs, double ys, double& lam, double& phi)
{
    if (p.oblique) {
        const double lamr = xs - p.lamp;
        const double coslam = cos(lamr), sinphi = sin(ys), cosphi = cos(ys);
        double s = p.sphip * sinphi + p.cphip * cosphi * coslam;
        s = s > 1 ? 1 : (s < -1 ? -1 : s);
        phi = asin(s);
        lam = atan2(cosphi * sin(lamr), p.sphip * cosphi * coslam - p.cphip * sinphi);
    } else {
        lam = xs - p.lamp;
        phi = ys;
    }
}

// geographic (rad) -> projected: pj_fwd.c around the projection's own function
__host__ __device__ inline void proj_forward(const ProjParams& p, double lon, double lat, double& x, double& y)
{
    if (p.kind == kLatLong) { x = lon; y = lat; return; }
    const double lam = adjlon(lon - p.lam0), phi = lat;
    double px = 0, py = 0;
    switch (p.kind) {
    case kStere: stere_forward(p, lam, phi, px, py); break;
    case kLcc: lcc_forward(p, lam, phi, px, py); break;
    case kMerc: merc_forward(p, lam, phi, px, py); break;
    case kTmerc: tmerc_forward(p, lam, phi, px, py); break;
    case kSinu: sinu_forward(p, lam, phi, px, py); break;
    case kCea: cea_forward(p, lam, phi, px, py); break;
    case kOrtho: ortho_forward(p, lam, phi, px, py); break;
    case kAeqd: aeqd_forward(p, lam, phi, px, py); break;
    case kNsper: nsper_forward(p, lam, phi, px, py); break;
    case kOmerc: omerc_forward(p, lam, phi, px, py); break;
    case kGeos: geos_forward(p, lam, phi, px, py); break;
    case kAea: aea_forward(p, lam, phi, px, py); break;
    case kLaea: laea_forward(p, lam, phi, px, py); break;
    case kEtmerc: etmerc_forward(p, lam, phi, px, py); break;
    default:  // kObTran: no radius, no unit
        ob_tran_forward(p, lam, phi, px, py);
        x = px + p.x0;
        y = py + p.y0;
        return;
    }
    x = p.frMeter * (p.a * px + p.x0);
    y = p.frMeter * (p.a * py + p.y0);
}

// projected -> geographic (rad): pj_inv.c around the projection's own function
__host__ __device__ inline void proj_inverse(const ProjParams& p, double x, double y, double& lon, double& lat)
{
    if (p.kind == kLatLong) { lon = x; lat = y; return; }
    double xs, ys;
    if (p.kind == kObTran) { xs = x - p.x0; ys = y - p.y0; }
    else { xs = (x * p.toMeter - p.x0) / p.a; ys = (y * p.toMeter - p.y0) / p.a; }
    double lam = 0, phi = 0;
    switch (p.kind) {
    case kStere: stere_inverse(p, xs, ys, lam, phi); break;
    case kLcc: lcc_inverse(p, xs, ys, lam, phi); break;
    case kMerc: merc_inverse(p, xs, ys, lam, phi); break;
    case kTmerc: tmerc_inverse(p, xs, ys, lam, phi); break;
    case kSinu: sinu_inverse(p, xs, ys, lam, phi); break;
    case kCea: cea_inverse(p, xs, ys, lam, phi); break;
    case kOrtho: ortho_inverse(p, xs, ys, lam, phi); break;
    case kAeqd: aeqd_inverse(p, xs, ys, lam, phi); break;
    case kNsper: nsper_inverse(p, xs, ys, lam, phi); break;
    case kOmerc: omerc_inverse(p, xs, ys, lam, phi); break;
    case kGeos: geos_inverse(p, xs, ys, lam, phi); break;
    case kAea: aea_inverse(p, xs, ys, lam, phi); break;
    case kLaea: laea_inverse(p, xs, ys, lam, phi); break;
    case kEtmerc: etmerc_inverse(p, xs, ys, lam, phi); break;
    default: ob_tran_inverse(p, xs, ys, lam, phi); break;
    }
    lon = adjlon(lam + p.lam0);
    lat = phi;
}

// geodetic (height 0) -> geocentric -> WGS84 -> the other datum -> geodetic (pj_datum_transform, pj_geocentric_to_wgs84 /
// _from_wgs84, geocent.c's iteration: at most 30 rounds, 1e-12)
__host__ __device__ inline void datum_shift(const ProjParams& src, const ProjParams& dst, double& lon, double& lat)
{
    const double sinlat = sin(lat), coslat = cos(lat);
    const double Rn = src.a / sqrt(1.0 - src.es * sinlat * sinlat);
    double X = Rn * coslat * cos(lon), Y = Rn * coslat * sin(lon), Z = (Rn * (1 - src.es)) * sinlat;
    const double* v = src.towgs84;
    if (src.datumType == 1) { X += v[0]; Y += v[1]; Z += v[2]; }
    else if (src.datumType == 2) {
        const double xo = v[6] * (X - v[5] * Y + v[4] * Z) + v[0], yo = v[6] * (v[5] * X + Y - v[3] * Z) + v[1],
                     zo = v[6] * (-v[4] * X + v[3] * Y + Z) + v[2];
        X = xo; Y = yo; Z = zo;
    }
    v = dst.towgs84;
    if (dst.datumType == 1) { X -= v[0]; Y -= v[1]; Z -= v[2]; }
    else if (dst.datumType == 2) {
        const double xt = (X - v[0]) / v[6], yt = (Y - v[1]) / v[6], zt = (Z - v[2]) / v[6];
        X = xt + v[5] * yt - v[4] * zt;
        Y = -v[5] * xt + yt + v[3] * zt;
        Z = v[4] * xt - v[3] * yt + zt;
    }
    // pj_Convert_Geocentric_To_Geodetic
    const double a = dst.a, es = dst.es, P = sqrt(X * X + Y * Y), RR = sqrt(X * X + Y * Y + Z * Z);
    if (P / a < 1.E-12) {
        lon = 0.;
        if (RR / a < 1.E-12) { lat = kHalfPi; return; }
    } else {
        lon = atan2(Y, X);
    }
    const double CT = Z / RR, ST = P / RR;
    double RX = 1.0 / sqrt(1.0 - es * (2.0 - es) * ST * ST);
    double CPHI0 = ST * (1.0 - es) * RX, SPHI0 = CT * RX, CPHI, SPHI, SDPHI;
    int iter = 0;
    do {
        ++iter;
        const double RN = a / sqrt(1.0 - es * SPHI0 * SPHI0);
        const double Height = P * CPHI0 + Z * SPHI0 - RN * (1.0 - es * SPHI0 * SPHI0);
        const double RK = es * RN / (RN + Height);
        RX = 1.0 / sqrt(1.0 - RK * (2.0 - RK) * ST * ST);
        CPHI = ST * (1.0 - RK) * RX;
        SPHI = CT * RX;
        SDPHI = SPHI * CPHI0 - CPHI * SPHI0;
        CPHI0 = CPHI;
        SPHI0 = SPHI;
    } while (SDPHI * SDPHI > 1.E-24 && iter < 30);
    lat = atan(SPHI / fabs(CPHI));
}

// pj_transform(src, dst) on one point
FA_HD void transform_point(const ProjParams& src, const ProjParams& dst, double& x, double& y)
{
    double lon, lat;
    proj_inverse(src, x, y, lon, lat);
    lon += src.fromGreenwich;  // pj_transform.c: longitudes meet relative to Greenwich
    if (src.doShift) datum_shift(src, dst, lon, lat);
    lon -= dst.fromGreenwich;
    proj_forward(dst, lon, lat, x, y);
}

// interpolation.c:311-329
FA_HD double bearing(double lat0, double lon0, double lat1, double lon1)
{
    const double dlon = lon0 - lon1;
    return atan2(sin(dlon) * cos(lat1), cos(lat0) * sin(lat1) - sin(lat0) * cos(lat1) * cos(dlon));
}

// mifi_get_vector_reproject_matrix_points_proj_delta (interpolation.c:330-438) on one point: the angle of the input projection's
// x direction (and y direction) seen in the output projection, from two finite differences.  (inX, inY) and (outX, outY) are the
// point in the two projections; m: the four entries of its matrix.
FA_HD void vector_matrix_point(const ProjParams& in, const ProjParams& out, double inX, double inY, double outX, double outY,
                               double deltaX, double deltaY, int outIsLatLong, double m[4])
{
    double ax = inX + deltaX, ay = inY;  // (x + d, y), :343-355
    double bx = inX, by = inY + deltaY;  // (x, y + d), :384-396
    transform_point(in, out, ax, ay);
    transform_point(in, out, bx, by);
    double phi0;
    if (outIsLatLong) {
        phi0 = bearing(outY, outX, by, bx);  // :408-412
        if (deltaY < 0) phi0 += kPi;
    } else {
        double phiy = atan2(ay - outY, ax - outX);  // :372-373
        if (deltaX < 0) phiy += kPi;
        double phix = -1 * atan2(bx - outX, by - outY);  // :414-415
        if (deltaY < 0) phix += kPi;
        phi0 = .5 * (phix + phiy);  // :424
    }
    const double c = cos(phi0), s = sin(phi0);
    m[0] = c;  // :429-432
    m[1] = s;
    m[2] = -1 * s;
    m[3] = phi0;
}

// reduceLatLonBoundingBox (src/CDMExtractor.cc:484-511) on one point of the mesh: transformed to degrees (Projection.cc:92-108),
// is it inside the box?  A point whose transformation fails is NaN and lies outside every box (divergence D10).
FA_HD bool inside_bounding_box(const ProjParams& src, const ProjParams& dst, double x, double y, double south, double north, double west,
                               double east)
{
    const bool wrap180 = west > east;  // :449
    double lon = x, lat = y;
    transform_point(src, dst, lon, lat);
    lon *= kRadToDeg;
    lat *= kRadToDeg;
    return __builtin_isfinite(lon) && __builtin_isfinite(lat) && !(lat < south || lat > north) &&
           (wrap180 ? !(lon > east && lon < west) : !(lon < west || lon > east));  // :501-506
}

// the delta of mifi_get_vector_reproject_matrix_proj (:458-518): 0.1 % of the distance between neighbouring cells, at the origin
// and in the middle of the mesh, both taken from the x field in the input projection as the reference does; at(i) reads cell i.
// Divergence D7: the second probe, cell (ox/2 + 1, oy/2 + 1), lies past the mesh when oy == 2, or ox == 2 and oy <= 4; the
// reference reads beyond the field there (:469), here the first probe stands alone.  Host side: at() may wait for the device.
template <class At>
double mesh_delta(At at, size_t ox, size_t oy)
{
    const double d = 1e-3;
    double delta;
    if (ox > 1 && oy > 1) {
        const size_t ox2 = ox / 2, oy2 = oy / 2;
        delta = d * (at(ox + 1) - at(0));
        const size_t far = (oy2 + 1) * ox + ox2 + 1;
        if (far < ox * oy) {
            delta += d * (at(far) - at(oy2 * ox + ox2));
            delta /= 2;
        }
    } else if (ox > 1) {
        delta = d * (at(1) - at(0));
    } else if (oy > 1) {
        delta = d * (at(ox) - at(0));
    } else {
        const double v = at(0);
        delta = (v > 1) ? v * d : d;
    }
    return std::fabs(delta) < 1e-9 ? d : delta;  // :509-513
}

}  // namespace fimex_amd
