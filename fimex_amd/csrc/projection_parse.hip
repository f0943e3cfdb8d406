// PROJ.4 strings to ProjParams (pj_init of PROJ.4 4.x); host code only, no kernel and no HIP call.
//
// Supported: latlong / longlat / latlon / lonlat, stere, lcc, merc, tmerc, etmerc, utm, laea, aea, geos, omerc (central point and
// azimuth), sinu, cea, ortho, aeqd, nsper and ob_tran with +o_proj=longlat +o_lat_p; on the sphere (+R) and -- except ob_tran,
// ortho, aeqd, nsper and the equatorial stereographic, where PROJ.4 releases differ -- on an ellipsoid given by +ellps,
// +datum=WGS84|NAD83|GGRS87|potsdam, or +a with +es, +e, +rf, +f or +b.  +units / +to_meter scale the projected coordinates as
// pj_fwd / pj_inv do (not with ob_tran), +pm shifts longitudes as pj_transform does, +axis=enu is accepted.  Geodetic coordinates
// pass unchanged between the two sides of a pair unless both name a datum (+datum, +towgs84) and the two differ: then
// pj_datum_transform's three- or seven-parameter shift is applied at height 0.
//
// Refused, each with a message that names the reason and repeats the string: +geoc, +over, +vto_meter, grid shifts (+nadgrids,
// +geoidgrids), the +R_A family, another +axis, unknown units, meridians, datums and ellipsoids, and every other projection.
#include "proj_math.hpp"

#include <map>
#include <sstream>
#include <string>

namespace fimex_amd {

namespace {

// the parameters of one string: +key=value or +key, the last of a repeated key wins
struct Args {
    std::string proj4;
    std::map<std::string, std::string> par;

    explicit Args(const char* text) : proj4(text)
    {
        std::istringstream in(proj4);
        std::string tok;
        while (in >> tok) {
            while (!tok.empty() && tok[0] == '+') tok.erase(0, 1);
            if (tok.empty()) continue;
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) par[tok] = "";
            else par[tok.substr(0, eq)] = tok.substr(eq + 1);
        }
    }
    bool has(const char* k) const { return par.count(k) != 0; }
    const std::string& str(const char* k) const { return par.at(k); }  // of a key that is there
    void set(const char* k, const std::string& v) { par[k] = v; }      // what a datum or an ellipsoid implies
    double num(const char* k, double d) const
    {
        auto it = par.find(k);
        if (it == par.end()) return d;
        try { return std::stod(it->second); } catch (...) { refuse("projection parameter +" + std::string(k) + " is not a number"); }
    }
    double rad(const char* k, double d) const { return has(k) ? num(k, 0) * kPi / 180.0 : d; }
    [[noreturn]] void refuse(const std::string& why) const { throw Error(why + ": " + proj4); }
};

bool geographic_name(const std::string& n) { return n == "latlong" || n == "longlat" || n == "latlon" || n == "lonlat"; }

// ---- what every projection shares ----

// pj_init: +to_meter=<number>[/<number>] wins over +units=<name> (pj_units.c)
void parse_units(ProjParams& p, const Args& a)
{
    p.toMeter = 1;
    if (a.has("to_meter") || a.has("units")) {
        std::string v;
        if (a.has("to_meter")) v = a.str("to_meter");
        else {
            static const struct { const char* id; const char* toMeter; } kUnits[] = {
                {"km", "1000."}, {"m", "1."}, {"dm", "1/10"}, {"cm", "1/100"}, {"mm", "1/1000"}, {"kmi", "1852.0"}, {"in", "0.0254"},
                {"ft", "0.3048"}, {"yd", "0.9144"}, {"mi", "1609.344"}, {"fath", "1.8288"}, {"ch", "20.1168"}, {"link", "0.201168"},
                {"us-in", "1./39.37"}, {"us-ft", "0.304800609601219"}, {"us-yd", "0.914401828803658"}, {"us-ch", "20.11684023368047"},
                {"us-mi", "1609.347218694437"}, {"ind-yd", "0.91439523"}, {"ind-ft", "0.30479841"}, {"ind-ch", "20.11669506"}};
            for (const auto& u : kUnits)
                if (a.str("units") == u.id) v = u.toMeter;
            if (v.empty()) a.refuse("unknown +units");
        }
        try {
            size_t used = 0;
            p.toMeter = std::stod(v, &used);
            if (used < v.size() && v[used] == '/') p.toMeter /= std::stod(v.substr(used + 1));
        } catch (...) { a.refuse("+to_meter is not a number"); }
        if (!(p.toMeter > 0)) a.refuse("invalid +to_meter");
    }
    p.frMeter = 1. / p.toMeter;
}

// pj_init: +pm is a name of pj_prime_meridians or an angle (here: decimal degrees, positive east)
void parse_prime_meridian(ProjParams& p, const Args& a)
{
    if (!a.has("pm")) return;
    static const struct { const char* id; double deg; } kMeridians[] = {
        {"greenwich", 0.}, {"lisbon", -(9 + 7 / 60. + 54.862 / 3600.)}, {"paris", 2 + 20 / 60. + 14.025 / 3600.},
        {"bogota", -(74 + 4 / 60. + 51.3 / 3600.)}, {"madrid", -(3 + 41 / 60. + 16.58 / 3600.)}, {"rome", 12 + 27 / 60. + 8.4 / 3600.},
        {"bern", 7 + 26 / 60. + 22.5 / 3600.}, {"jakarta", 106 + 48 / 60. + 27.79 / 3600.}, {"ferro", -(17 + 40 / 60.)},
        {"brussels", 4 + 22 / 60. + 4.71 / 3600.}, {"stockholm", 18 + 3 / 60. + 29.8 / 3600.}, {"athens", 23 + 42 / 60. + 58.815 / 3600.},
        {"oslo", 10 + 43 / 60. + 22.5 / 3600.}};
    const std::string& pm = a.str("pm");
    for (const auto& m : kMeridians)
        if (pm == m.id) { p.fromGreenwich = m.deg * kPi / 180.0; return; }
    size_t used = 0;
    double deg = 0;
    try { deg = std::stod(pm, &used); } catch (...) { used = 0; }
    if (used == 0 || used != pm.size()) a.refuse("+pm is neither a known meridian nor decimal degrees");
    p.fromGreenwich = deg * kPi / 180.0;
}

// pj_datum_set: +towgs84, or the one a +datum of pj_datums.c implies (entries without a grid)
void parse_datum(ProjParams& p, Args& a)
{
    p.datum = a.has("datum") || a.has("towgs84");
    if (a.has("datum") && !a.has("towgs84")) {
        const std::string& d = a.str("datum");
        if (d == "WGS84" || d == "NAD83") a.set("towgs84", "0,0,0");
        else if (d == "GGRS87") a.set("towgs84", "-199.87,74.79,246.62");
        else if (d == "potsdam") a.set("towgs84", "598.1,73.7,418.2,0.202,0.045,-2.455,6.7");
        else a.refuse("datum not implemented");
    }
    if (!a.has("towgs84")) return;
    std::istringstream list(a.str("towgs84"));
    std::string item;
    for (int i = 0; i < 7 && std::getline(list, item, ','); ++i) {
        try { p.towgs84[i] = std::stod(item); } catch (...) { a.refuse("+towgs84 is not a list of numbers"); }
    }
    if (p.towgs84[3] != 0 || p.towgs84[4] != 0 || p.towgs84[5] != 0 || p.towgs84[6] != 0) {
        p.datumType = 2;
        for (int i = 3; i < 6; ++i) p.towgs84[i] *= 4.84813681109535993589914102357e-6;  // SEC_TO_RAD
        p.towgs84[6] = p.towgs84[6] / 1000000.0 + 1;
    } else p.datumType = 1;
}

struct Ellipsoid { const char* name; double a; bool byB; double shape; };  // pj_ellps.c
constexpr Ellipsoid kEllipsoids[] = {
    {"sphere", 6370997.0, true, 6370997.0},  {"WGS84", 6378137.0, false, 298.257223563}, {"GRS80", 6378137.0, false, 298.257222101},
    {"WGS72", 6378135.0, false, 298.26},     {"GRS67", 6378160.0, false, 298.2471674270}, {"bessel", 6377397.155, false, 299.1528128},
    {"intl", 6378388.0, false, 297.},        {"clrk66", 6378206.4, true, 6356583.8},      {"clrk80", 6378249.145, false, 293.4663},
    {"krass", 6378245.0, false, 298.3},      {"airy", 6377563.396, true, 6356256.910},      {"evrstSS", 6377298.556, false, 300.8017},
};

// pj_ell_set: +R, or an explicit +a wins over the one +ellps implies; the shape is the first of +es +e +rf +f +b
void parse_ellipsoid(ProjParams& p, Args& a)
{
    p.a = 1;
    if (a.has("R")) { p.a = a.num("R", 1); return; }
    if (a.has("datum") && !a.has("ellps")) {
        const std::string& d = a.str("datum");
        if (d == "WGS84") a.set("ellps", "WGS84");
        else if (d == "NAD83" || d == "GGRS87") a.set("ellps", "GRS80");
        else if (d == "potsdam") a.set("ellps", "bessel");
        else a.refuse("datum not implemented");
    }
    if (a.has("ellps")) {
        const Ellipsoid* ell = nullptr;
        for (const Ellipsoid& cand : kEllipsoids)
            if (a.str("ellps") == cand.name) ell = &cand;
        if (!ell) a.refuse("ellipsoid not implemented");
        char buf[64];
        if (!a.has("a")) { std::snprintf(buf, sizeof buf, "%.17g", ell->a); a.set("a", buf); }
        if (!a.has("es") && !a.has("e") && !a.has("rf") && !a.has("f") && !a.has("b")) {
            std::snprintf(buf, sizeof buf, "%.17g", ell->shape);
            a.set(ell->byB ? "b" : "rf", buf);
        }
    }
    if (a.has("a")) {
        p.a = a.num("a", 1);
        if (a.has("es")) p.es = a.num("es", 0);
        else if (a.has("e")) { p.es = a.num("e", 0); p.es *= p.es; }
        else if (a.has("rf")) { p.es = 1. / a.num("rf", 1); p.es = p.es * (2. - p.es); }
        else if (a.has("f")) { p.es = a.num("f", 0); p.es = p.es * (2. - p.es); }
        else if (a.has("b")) { const double b = a.num("b", 1); p.es = 1. - (b * b) / (p.a * p.a); }
        if (!(p.a > 0) || p.es < 0 || p.es >= 1) a.refuse("invalid ellipsoid");
    } else if (!geographic_name(a.str("proj"))) {
        a.refuse("projection string without an ellipsoid (+R, +a or +ellps)");
    }
}

// ---- series coefficients ----

// pj_enfn: the meridional distance
void enfn(double es, double* en)
{
    constexpr double C00 = 1., C02 = .25, C04 = .046875, C06 = .01953125, C08 = .01068115234375, C22 = .75, C44 = .46875,
                     C46 = .01302083333333333333, C48 = .00712076822916666666, C66 = .36458333333333333333,
                     C68 = .00569661458333333333, C88 = .3076171875;
    double t;
    en[0] = C00 - es * (C02 + es * (C04 + es * (C06 + es * C08)));
    en[1] = es * (C22 - es * (C04 + es * (C06 + es * C08)));
    en[2] = (t = es * es) * (C44 - es * (C46 + es * C48));
    en[3] = (t *= es) * (C66 - es * C68);
    en[4] = t * es * C88;
}

// pj_authset: the authalic latitude's series
void authset(double es, double* apa)
{
    double t = es * es;
    apa[0] = es * .33333333333333333333 + t * .17222222222222222222;
    apa[1] = t * .06388888888888888888;
    t *= es;
    apa[0] += t * .10257936507936507936;
    apa[1] += t * .06640211640211640211;
    apa[2] = t * .01641501294219154443;
}

// PJ_etmerc.c: Clenshaw summation of the real sine series
double clens(const double* a, double argR)
{
    const double r = 2 * std::cos(argR);
    double hr = a[5], hr1 = 0, hr2;
    for (int k = 4; k >= 0; --k) {
        hr2 = hr1;
        hr1 = hr;
        hr = -hr2 + r * hr1 + a[k];
    }
    return std::sin(argR) * hr;
}

// Engsager & Poder's series to the sixth power of the third flattening (PJ_etmerc.c setup)
void etmerc_series(ProjParams& p)
{
    const double f = p.es / (1 + std::sqrt(1 - p.es));
    const double n = f / (2 - f);
    double np = n;
    p.cgb[0] = n * (2 + n * (-2 / 3.0 + n * (-2 + n * (116 / 45.0 + n * (26 / 45.0 + n * (-2854 / 675.0))))));
    p.cbg[0] = n * (-2 + n * (2 / 3.0 + n * (4 / 3.0 + n * (-82 / 45.0 + n * (32 / 45.0 + n * (4642 / 4725.0))))));
    np *= n;
    p.cgb[1] = np * (7 / 3.0 + n * (-8 / 5.0 + n * (-227 / 45.0 + n * (2704 / 315.0 + n * (2323 / 945.0)))));
    p.cbg[1] = np * (5 / 3.0 + n * (-16 / 15.0 + n * (-13 / 9.0 + n * (904 / 315.0 + n * (-1522 / 945.0)))));
    np *= n;
    p.cgb[2] = np * (56 / 15.0 + n * (-136 / 35.0 + n * (-1262 / 105.0 + n * (73814 / 2835.0))));
    p.cbg[2] = np * (-26 / 15.0 + n * (34 / 21.0 + n * (8 / 5.0 + n * (-12686 / 2835.0))));
    np *= n;
    p.cgb[3] = np * (4279 / 630.0 + n * (-332 / 35.0 + n * (-399572 / 14175.0)));
    p.cbg[3] = np * (1237 / 630.0 + n * (-12 / 5.0 + n * (-24832 / 14175.0)));
    np *= n;
    p.cgb[4] = np * (4174 / 315.0 + n * (-144838 / 6237.0));
    p.cbg[4] = np * (-734 / 315.0 + n * (109598 / 31185.0));
    np *= n;
    p.cgb[5] = np * (601676 / 22275.0);
    p.cbg[5] = np * (444337 / 155925.0);
    np = n * n;
    p.Qn = p.k0 / (1 + n) * (1 + np * (1 / 4.0 + np * (1 / 64.0 + np / 256.0)));
    p.utg[0] = n * (-0.5 + n * (2 / 3.0 + n * (-37 / 96.0 + n * (1 / 360.0 + n * (81 / 512.0 + n * (-96199 / 604800.0))))));
    p.gtu[0] = n * (0.5 + n * (-2 / 3.0 + n * (5 / 16.0 + n * (41 / 180.0 + n * (-127 / 288.0 + n * (7891 / 37800.0))))));
    p.utg[1] = np * (-1 / 48.0 + n * (-1 / 15.0 + n * (437 / 1440.0 + n * (-46 / 105.0 + n * (1118711 / 3870720.0)))));
    p.gtu[1] = np * (13 / 48.0 + n * (-3 / 5.0 + n * (557 / 1440.0 + n * (281 / 630.0 + n * (-1983433 / 1935360.0)))));
    np *= n;
    p.utg[2] = np * (-17 / 480.0 + n * (37 / 840.0 + n * (209 / 4480.0 + n * (-5569 / 90720.0))));
    p.gtu[2] = np * (61 / 240.0 + n * (-103 / 140.0 + n * (15061 / 26880.0 + n * (167603 / 181440.0))));
    np *= n;
    p.utg[3] = np * (-4397 / 161280.0 + n * (11 / 504.0 + n * (830251 / 7257600.0)));
    p.gtu[3] = np * (49561 / 161280.0 + n * (-179 / 168.0 + n * (6601661 / 7257600.0)));
    np *= n;
    p.utg[4] = np * (-4583 / 161280.0 + n * (108847 / 3991680.0));
    p.gtu[4] = np * (34729 / 80640.0 + n * (-3418889 / 1995840.0));
    np *= n;
    p.utg[5] = np * (-20648693 / 638668800.0);
    p.gtu[5] = np * (212378941 / 319334400.0);
    const double Z = gatg(p.cbg, p.phi0);
    p.Zb = -p.Qn * (Z + clens(p.gtu, 2 * Z));
}

// ---- one set-up per projection: the common part has filled a, es, e, lam0, phi0, x0, y0, k0, the units and the datum ----

// the aspect of laea, ortho, aeqd and nsper (stere draws the line at kEps10 the other way, see setup_stere)
int aspect_of(double phi0)
{
    const double t = std::fabs(phi0);
    if (std::fabs(t - kHalfPi) < kEps10) return phi0 < 0 ? kSouth : kNorth;
    return t < kEps10 ? kEquatorial : kOblique;
}

void setup_stere(ProjParams& p, const Args& a)  // PJ_stere.c
{
    const double phits = a.has("lat_ts") ? std::fabs(a.rad("lat_ts", kHalfPi)) : kHalfPi;
    const double t = std::fabs(p.phi0);
    if (std::fabs(t - kHalfPi) < kEps10) p.mode = p.phi0 < 0 ? kSouth : kNorth;
    else p.mode = t > kEps10 ? kOblique : kEquatorial;
    if (p.es != 0) {
        if (p.mode == kEquatorial) a.refuse("the equatorial stereographic projection is implemented on the sphere only");
        if (p.mode == kNorth || p.mode == kSouth) {
            if (std::fabs(phits - kHalfPi) < kEps10) p.akm1 = 2. * p.k0 / std::sqrt(std::pow(1 + p.e, 1 + p.e) * std::pow(1 - p.e, 1 - p.e));
            else {
                double t = std::sin(phits);
                p.akm1 = std::cos(phits) / tsfn(phits, t, p.e);
                t *= p.e;
                p.akm1 /= std::sqrt(1. - t * t);
            }
        } else {
            double t = std::sin(p.phi0);
            const double X = 2. * std::atan(ssfn(p.phi0, t, p.e)) - kHalfPi;
            t *= p.e;
            p.akm1 = 2. * p.k0 * std::cos(p.phi0) / std::sqrt(1. - t * t);
            p.sinph0 = std::sin(X);
            p.cosph0 = std::cos(X);
        }
    } else if (p.mode == kNorth || p.mode == kSouth) {
        p.akm1 = (std::fabs(phits - kHalfPi) >= kEps10) ? std::cos(phits) / std::tan(kFortPi - .5 * phits) : 2. * p.k0;
    } else {
        p.sinph0 = std::sin(p.phi0);
        p.cosph0 = std::cos(p.phi0);
        p.akm1 = 2. * p.k0;
    }
}

void setup_lcc(ProjParams& p, const Args& a)  // PJ_lcc.c
{
    const double phi1 = a.rad("lat_1", 0);
    const double phi2 = a.has("lat_2") ? a.rad("lat_2", phi1) : phi1;
    if (!a.has("lat_0")) p.phi0 = phi1;
    if (std::fabs(phi1 + phi2) < kEps10) a.refuse("lcc: lat_1 = -lat_2");
    const double sinphi = std::sin(phi1), cosphi = std::cos(phi1);
    const bool secant = std::fabs(phi1 - phi2) >= kEps10;
    p.n = sinphi;
    if (p.es != 0) {
        const double m1 = msfn(sinphi, cosphi, p.es), ml1 = tsfn(phi1, sinphi, p.e);
        if (secant) {
            const double sinphi2 = std::sin(phi2);
            p.n = std::log(m1 / msfn(sinphi2, std::cos(phi2), p.es));
            p.n /= std::log(ml1 / tsfn(phi2, sinphi2, p.e));
        }
        p.c = p.rho0 = m1 * std::pow(ml1, -p.n) / p.n;
        p.rho0 *= (std::fabs(std::fabs(p.phi0) - kHalfPi) < kEps10) ? 0. : std::pow(tsfn(p.phi0, std::sin(p.phi0), p.e), p.n);
    } else {
        if (secant) p.n = std::log(cosphi / std::cos(phi2)) / std::log(std::tan(kFortPi + .5 * phi2) / std::tan(kFortPi + .5 * phi1));
        p.c = cosphi * std::pow(std::tan(kFortPi + .5 * phi1), p.n) / p.n;
        p.rho0 = (std::fabs(std::fabs(p.phi0) - kHalfPi) < kEps10) ? 0. : p.c * std::pow(std::tan(kFortPi + .5 * p.phi0), -p.n);
    }
}

void setup_merc(ProjParams& p, const Args& a)  // PJ_merc.c
{
    if (!a.has("lat_ts")) return;
    const double phits = std::fabs(a.rad("lat_ts", 0));
    if (phits >= kHalfPi) a.refuse("merc: lat_ts >= 90");
    p.k0 = p.es != 0 ? msfn(std::sin(phits), std::cos(phits), p.es) : std::cos(phits);
}

void setup_tmerc(ProjParams& p, const Args&)  // PJ_tmerc.c (4.x)
{
    if (p.es != 0) {
        enfn(p.es, p.en);
        p.ml0 = mlfn(p.phi0, std::sin(p.phi0), std::cos(p.phi0), p.en);
        p.esp = p.es / (1. - p.es);
    } else {
        p.esp = p.k0;
        p.ml0 = .5 * p.esp;
    }
}

void setup_etmerc(ProjParams& p, const Args& a)  // PJ_etmerc.c
{
    if (p.es == 0) a.refuse("etmerc needs an ellipsoid");
    etmerc_series(p);
}

// utm is etmerc since PROJ.4 4.9.3 (the release debian_bionic/control builds against) and tmerc before; the two differ by
// < 1 mm within 6 degrees of the meridian, but only etmerc inverts itself far from it
void setup_utm(ProjParams& p, const Args& a)  // PJ_tmerc.c / PJ_etmerc.c, utm entry
{
    if (p.es == 0) a.refuse("utm needs an ellipsoid");
    p.y0 = a.has("south") ? 10000000. : 0.;
    p.x0 = 500000.;
    long zone;
    if (a.has("zone")) {
        zone = (long)a.num("zone", 0);
        if (zone < 1 || zone > 60) a.refuse("invalid UTM zone");
        --zone;
    } else {
        double l = p.lam0;
        if (std::fabs(l) > kSpi) { l += kPi; l -= 2 * kPi * std::floor(l / (2 * kPi)); l -= kPi; }
        zone = (long)std::floor((l + kPi) * 30. / kPi);
        zone = zone < 0 ? 0 : (zone >= 60 ? 59 : zone);
    }
    p.lam0 = (zone + .5) * kPi / 30. - kPi;
    p.k0 = 0.9996;
    p.phi0 = 0.;
    setup_etmerc(p, a);
}

void setup_sinu(ProjParams& p, const Args&)  // PJ_gn_sinu.c
{
    if (p.es != 0) enfn(p.es, p.en);
}

void setup_cea(ProjParams& p, const Args& a)  // PJ_cea.c
{
    const double t = a.rad("lat_ts", 0);
    p.k0 = std::cos(t);
    if (p.k0 < 0) a.refuse("cea: |lat_ts| > 90");
    if (p.es != 0) {
        const double st = std::sin(t);
        p.k0 /= std::sqrt(1. - p.es * st * st);
        authset(p.es, p.apa);
        p.qp = qsfn(1., p.e, 1. - p.es);
    }
}

void setup_sphere_azimuthal(ProjParams& p, const Args& a)  // PJ_ortho.c, PJ_aeqd.c (sphere), and the start of PJ_nsper.c
{
    if (p.es != 0) a.refuse(a.str("proj") + " is implemented on the sphere only");
    p.mode = aspect_of(p.phi0);
    p.sinph0 = std::sin(p.phi0);
    p.cosph0 = std::cos(p.phi0);
}

void setup_nsper(ProjParams& p, const Args& a)  // PJ_nsper.c
{
    setup_sphere_azimuthal(p, a);
    const double height = a.num("h", 0);
    if (!(height > 0)) a.refuse("nsper needs +h > 0");
    p.pn1 = height / p.a;
    p.pp = 1. + p.pn1;
    p.rp = 1. / p.pp;
    p.pfact = (p.pp + 1.) / p.pn1;
}

void setup_omerc(ProjParams& p, const Args& a)  // PJ_omerc.c, central point and azimuth (Snyder's alternate B)
{
    const bool alp = a.has("alpha"), gam = a.has("gamma");
    if (!alp && !gam) a.refuse("omerc is implemented by central point and azimuth (+lonc +alpha / +gamma) only");
    p.mode = a.has("no_rot");
    const bool no_off = a.has("no_off") || a.has("no_uoff");
    double alpha_c = a.rad("alpha", 0), gamma = a.rad("gamma", 0), gamma0;
    const double lamc = a.rad("lonc", 0), com = std::sqrt(1. - p.es);
    double D, F;
    if (std::fabs(p.phi0) > kEps10) {
        const double sinph0 = std::sin(p.phi0), cosph0 = std::cos(p.phi0);
        const double con = 1. - p.es * sinph0 * sinph0;
        p.oB = cosph0 * cosph0;
        p.oB = std::sqrt(1. + p.es * p.oB * p.oB / (1. - p.es));
        p.oA = p.oB * p.k0 * com / con;
        D = p.oB * com / (cosph0 * std::sqrt(con));
        if ((F = D * D - 1.) <= 0.) F = 0.;
        else {
            F = std::sqrt(F);
            if (p.phi0 < 0.) F = -F;
        }
        p.oE = F += D;
        p.oE *= std::pow(tsfn(p.phi0, sinph0, p.e), p.oB);
    } else {
        p.oB = 1. / com;
        p.oA = p.k0;
        p.oE = D = F = 1.;
    }
    if (alp) {
        gamma0 = std::asin(std::sin(alpha_c) / D);
        if (!gam) gamma = alpha_c;
    } else {
        alpha_c = std::asin(D * std::sin(gamma0 = gamma));
    }
    const double con = std::fabs(alpha_c);
    if (con <= 1e-7 || std::fabs(con - kPi) <= 1e-7 || std::fabs(std::fabs(p.phi0) - kHalfPi) <= 1e-7)
        a.refuse("omerc: alpha of 0 or 180 degrees, or lat_0 at a pole");
    p.lam0 = lamc - std::asin(.5 * (F - 1. / F) * std::tan(gamma0)) / p.oB;  // +lon_0 plays no role
    p.singam = std::sin(gamma0);
    p.cosgam = std::cos(gamma0);
    p.sinrot = std::sin(gamma);
    p.cosrot = std::cos(gamma);
    p.BrA = 1. / (p.ArB = p.oA * (p.rB = 1. / p.oB));
    if (no_off) p.u_0 = 0;
    else {
        p.u_0 = std::fabs(p.ArB * std::atan2(std::sqrt(D * D - 1.), std::cos(alpha_c)));
        if (p.phi0 < 0.) p.u_0 = -p.u_0;
    }
    p.v_pole_n = p.ArB * std::log(std::tan(kFortPi - .5 * gamma0));
    p.v_pole_s = p.ArB * std::log(std::tan(kFortPi + .5 * gamma0));
}

void setup_geos(ProjParams& p, const Args& a)  // PJ_geos.c
{
    const double h = a.num("h", 0);
    if (!(h > 0)) a.refuse("geos needs +h > 0");
    if (p.phi0 != 0) a.refuse("geos: lat_0 must be 0");
    p.mode = 0;
    if (a.has("sweep")) {
        if (a.str("sweep") != "x" && a.str("sweep") != "y") a.refuse("geos: +sweep must be x or y");
        p.mode = a.str("sweep") == "x";
    }
    p.radius_g_1 = h / p.a;
    p.radius_g = 1. + p.radius_g_1;
    p.C = p.radius_g * p.radius_g - 1.0;
    if (p.es != 0) {
        p.radius_p = std::sqrt(1. - p.es);
        p.radius_p2 = 1. - p.es;
        p.radius_p_inv2 = 1. / (1. - p.es);
    } else {
        p.radius_p = p.radius_p2 = p.radius_p_inv2 = 1.;
    }
}

void setup_aea(ProjParams& p, const Args& a)  // PJ_aea.c
{
    const double phi1 = a.rad("lat_1", 0), phi2 = a.rad("lat_2", 0);
    if (std::fabs(phi1 + phi2) < kEps10) a.refuse("aea: lat_1 = -lat_2");
    double sinphi = std::sin(phi1), cosphi = std::cos(phi1);
    p.n = sinphi;
    const bool secant = std::fabs(phi1 - phi2) >= kEps10;
    if (p.es != 0) {
        const double one_es = 1. - p.es;
        const double m1 = msfn(sinphi, cosphi, p.es), ml1 = qsfn(sinphi, p.e, one_es);
        if (secant) {
            sinphi = std::sin(phi2);
            cosphi = std::cos(phi2);
            const double m2 = msfn(sinphi, cosphi, p.es), ml2 = qsfn(sinphi, p.e, one_es);
            p.n = (m1 * m1 - m2 * m2) / (ml2 - ml1);
        }
        p.ec = 1. - .5 * one_es * std::log((1. - p.e) / (1. + p.e)) / p.e;
        p.c = m1 * m1 + p.n * ml1;
        p.dd = 1. / p.n;
        p.rho0 = p.dd * std::sqrt(p.c - p.n * qsfn(std::sin(p.phi0), p.e, one_es));
    } else {
        if (secant) p.n = .5 * (p.n + std::sin(phi2));
        p.n2 = p.n + p.n;
        p.c = cosphi * cosphi + p.n2 * sinphi;
        p.dd = 1. / p.n;
        p.rho0 = p.dd * std::sqrt(p.c - p.n2 * std::sin(p.phi0));
    }
}

void setup_laea(ProjParams& p, const Args&)  // PJ_laea.c
{
    p.mode = aspect_of(p.phi0);
    if (p.es != 0) {
        const double one_es = 1. - p.es;
        p.qp = qsfn(1., p.e, one_es);
        authset(p.es, p.apa);
        if (p.mode == kNorth || p.mode == kSouth) p.dd = 1.;
        else if (p.mode == kEquatorial) {
            p.rq = std::sqrt(.5 * p.qp);
            p.dd = 1. / p.rq;
            p.xmf = 1.;
            p.ymf = .5 * p.qp;
        } else {
            p.rq = std::sqrt(.5 * p.qp);
            const double sinphi = std::sin(p.phi0);
            p.sinb1 = qsfn(sinphi, p.e, one_es) / p.qp;
            p.cosb1 = std::sqrt(1. - p.sinb1 * p.sinb1);
            p.dd = std::cos(p.phi0) / (std::sqrt(1. - p.es * sinphi * sinphi) * p.rq * p.cosb1);
            p.ymf = (p.xmf = p.rq) / p.dd;
            p.xmf *= p.dd;
        }
    } else if (p.mode == kOblique) {
        p.sinb1 = std::sin(p.phi0);
        p.cosb1 = std::cos(p.phi0);
    }
}

void setup_ob_tran(ProjParams& p, const Args& a)  // PJ_ob_tran.c around longlat
{
    if (p.toMeter != 1) a.refuse("+units / +to_meter with ob_tran are not implemented");
    if (p.es != 0) a.refuse("ob_tran is implemented on the sphere only");
    if (!a.has("o_proj") || !geographic_name(a.str("o_proj")) || !a.has("o_lat_p"))
        a.refuse("ob_tran is implemented for +o_proj=longlat +o_lat_p only");
    p.lamp = a.rad("o_lon_p", 0);
    const double phip = a.rad("o_lat_p", kHalfPi);
    p.oblique = std::fabs(phip - kHalfPi) > kEps10;
    p.sphip = std::sin(phip);
    p.cphip = std::cos(phip);
}

constexpr struct { const char* name; ProjKind kind; void (*setup)(ProjParams&, const Args&); } kProjections[] = {
    {"latlong", kLatLong, nullptr}, {"longlat", kLatLong, nullptr}, {"latlon", kLatLong, nullptr}, {"lonlat", kLatLong, nullptr},
    {"stere", kStere, setup_stere}, {"lcc", kLcc, setup_lcc},       {"merc", kMerc, setup_merc},   {"tmerc", kTmerc, setup_tmerc},
    {"etmerc", kEtmerc, setup_etmerc}, {"utm", kEtmerc, setup_utm}, {"sinu", kSinu, setup_sinu},   {"cea", kCea, setup_cea},
    {"ortho", kOrtho, setup_sphere_azimuthal}, {"aeqd", kAeqd, setup_sphere_azimuthal}, {"nsper", kNsper, setup_nsper},
    {"omerc", kOmerc, setup_omerc}, {"geos", kGeos, setup_geos},    {"aea", kAea, setup_aea},      {"laea", kLaea, setup_laea},
    {"ob_tran", kObTran, setup_ob_tran},
};

}  // namespace

ProjParams parse_proj4(const char* text)
{
    FA_REQUIRE(text != nullptr, "NULL projection string");
    Args a(text);
    if (!a.has("proj")) a.refuse("projection string without +proj");
    for (const char* k : {"geoc", "over", "vto_meter", "nadgrids", "geoidgrids", "R_A", "R_V", "R_a", "R_g", "R_h", "R_lat_a", "R_lat_g"})
        if (a.has(k)) a.refuse("projection parameter +" + std::string(k) + " is not implemented");
    if (a.has("axis") && a.str("axis") != "enu") a.refuse("projection +axis other than enu is not implemented");
    ProjParams p{};
    parse_units(p, a);
    parse_prime_meridian(p, a);
    parse_datum(p, a);
    parse_ellipsoid(p, a);
    p.e = std::sqrt(p.es);
    if (p.datumType == 1 && p.towgs84[0] == 0 && p.towgs84[1] == 0 && p.towgs84[2] == 0 && p.a == 6378137.0 &&
        std::fabs(p.es - 0.006694379990) < 0.000000000050)
        p.datumType = 3;  // pj_init: PJD_WGS84
    p.lam0 = a.rad("lon_0", 0);
    p.phi0 = a.rad("lat_0", 0);
    p.x0 = a.num("x_0", 0);
    p.y0 = a.num("y_0", 0);
    p.k0 = a.has("k_0") ? a.num("k_0", 1) : a.num("k", 1);
    const std::string& name = a.str("proj");
    for (const auto& proj : kProjections) {
        if (name != proj.name) continue;
        p.kind = proj.kind;
        if (proj.setup) proj.setup(p, a);
        return p;
    }
    throw Error("projection not implemented: " + name);
}

ProjPair parse_pair(const char* projIn, const char* projOut)
{
    ProjPair pp{parse_proj4(projIn), parse_proj4(projOut)};
    const ProjParams &a = pp.src, &b = pp.dst;
    if (a.datumType != 0 && b.datumType != 0) {
        bool same = a.datumType == b.datumType && a.a == b.a && std::fabs(a.es - b.es) <= 0.000000000050;
        const int nPar = a.datumType == 1 ? 3 : (a.datumType == 2 ? 7 : 0);
        for (int i = 0; i < nPar; ++i) same = same && a.towgs84[i] == b.towgs84[i];
        const bool params = a.datumType == 1 || a.datumType == 2 || b.datumType == 1 || b.datumType == 2;
        pp.src.doShift = pp.dst.doShift = !same && (a.es != b.es || a.a != b.a || params);  // either side may be the source of a call
    }
    return pp;
}

}  // namespace fimex_amd
