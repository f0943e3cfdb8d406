"""The projection strings, point distributions and refusals that tests/test_gpu_projection.py (the library on the GPU) and
tests/test_projection_host.py (the same parser and point math compiled for the CPU) share."""
import numpy as np

from oracle import proj_oracle as po

GEO = "+proj=latlong +R=6371000"
STERE = "+proj=stere +lat_0=90 +lon_0=0 +lat_ts=60 +a=6371000 +e=0"
STERE_OBL = "+proj=stere +lat_0=52 +lon_0=10 +R=6371000 +x_0=1000 +y_0=-2000"
STERE_EQ = "+proj=stere +lat_0=0 +lon_0=-20 +R=6371000"
STERE_S = "+proj=stere +lat_0=-90 +lon_0=30 +lat_ts=-71 +R=6371000"
LCC = "+proj=lcc +lat_0=63 +lon_0=15 +lat_1=63 +lat_2=63 +no_defs +R=6.371e+06"
LCC2 = "+proj=lcc +lat_0=48 +lon_0=8 +lat_1=30 +lat_2=60 +R=6371229"
MERC = "+proj=merc +lon_0=5 +lat_ts=30 +R=6371000"
ROT = "+proj=ob_tran +o_proj=longlat +lon_0=-40 +o_lat_p=22 +R=6.371e+06 +no_defs"
LAEA_S = "+proj=laea +lat_0=52 +lon_0=10 +R=6371000"
LAEA_SP = "+proj=laea +lat_0=90 +lon_0=-30 +R=6371000 +x_0=100"
AEA_S = "+proj=aea +lat_1=40 +lat_2=60 +lat_0=50 +lon_0=10 +R=6371000"
SINU_S = "+proj=sinu +lon_0=10 +R=6371000"
CEA_S = "+proj=cea +lat_ts=30 +lon_0=-20 +R=6371000"
ORTHO = "+proj=ortho +lat_0=40 +lon_0=10 +R=6371000"
ORTHO_P = "+proj=ortho +lat_0=90 +lon_0=-30 +R=6371000"
AEQD = "+proj=aeqd +lat_0=40 +lon_0=10 +R=6371000"
AEQD_P = "+proj=aeqd +lat_0=90 +lon_0=0 +R=6371000"
NSPER = "+proj=nsper +h=2e7 +lat_0=50 +lon_0=10 +R=6371000"
ALL = [GEO, STERE, STERE_OBL, STERE_EQ, STERE_S, LCC, LCC2, MERC, ROT, LAEA_S, LAEA_SP, AEA_S, SINU_S, CEA_S, ORTHO, ORTHO_P, AEQD, AEQD_P, NSPER]
# on an ellipsoid (the UTM string is the one of test/testInterpolator.cc:422)
GEO_W = "+proj=latlong +datum=WGS84"
UTM33 = "+proj=utm +zone=33 +datum=WGS84 +no_defs"
ETMERC = "+proj=etmerc +lon_0=-3 +lat_0=49 +k=0.9996012717 +x_0=400000 +y_0=-100000 +ellps=airy"
UTM17S = "+proj=utm +zone=17 +south +ellps=GRS80"
TMERC_S = "+proj=tmerc +lon_0=12 +lat_0=0 +k=0.9996 +R=6371000"   # lat_0 != 0 on the sphere: PROJ.4 releases pick the hemisphere differently
TMERC_B = "+proj=tmerc +lon_0=9 +lat_0=0 +k=1 +x_0=3500000 +ellps=bessel"
STERE_W = "+proj=stere +lat_0=90 +lon_0=-45 +lat_ts=70 +ellps=WGS84"
STERE_WS = "+proj=stere +lat_0=-90 +lon_0=0 +lat_ts=-71 +ellps=WGS84"
STERE_WP = "+proj=stere +lat_0=90 +lon_0=10 +k=0.994 +ellps=intl"
STERE_WO = "+proj=stere +lat_0=52.156 +lon_0=5.387 +k=0.9999079 +x_0=155000 +y_0=463000 +ellps=bessel"
LCC_W = "+proj=lcc +lat_0=52 +lon_0=10 +lat_1=35 +lat_2=65 +x_0=4000000 +y_0=2800000 +ellps=GRS80"
LCC_W1 = "+proj=lcc +lat_0=63 +lon_0=15 +lat_1=63 +a=6378137 +rf=298.257223563"
MERC_W = "+proj=merc +lon_0=5 +lat_ts=30 +ellps=WGS84"
LAEA_W = "+proj=laea +lat_0=52 +lon_0=10 +x_0=4321000 +y_0=3210000 +ellps=GRS80"   # ETRS89-LAEA
LAEA_WP = "+proj=laea +lat_0=90 +lon_0=0 +ellps=WGS84"
LAEA_WE = "+proj=laea +lat_0=0 +lon_0=20 +ellps=WGS84"
AEA_W = "+proj=aea +lat_1=29.5 +lat_2=45.5 +lat_0=23 +lon_0=-96 +x_0=0 +y_0=0 +ellps=GRS80"
AEA_W1 = "+proj=aea +lat_1=55 +lat_2=55 +lat_0=50 +lon_0=10 +ellps=WGS84"
GEOS_MSG = "+proj=geos +lon_0=0 +h=3.57858e+07  +a=6.37817e+06  +b=6.35658e+06 +no_defs +x_0=-2.2098e+06 +y_0=-3.50297e+06"   # testProjections.cc:69
GEOS_X = "+proj=geos +lon_0=-75 +h=35786023 +sweep=x +ellps=GRS80"
OMERC_REF = "+proj=omerc +lonc=5.34065 +lat_0=60.742 +alpha=19.0198 +no_rot   +a=6.37814e+06  +b=6.35675e+06 +no_defs +x_0=-3.86098e+06 +y_0=1.5594e+06"   # testProjections.cc:56
OMERC_RSO = "+proj=omerc +lat_0=4 +lonc=115 +alpha=53.31582047222222 +gamma=53.13010236111111 +k=0.99984 +x_0=590476.87 +y_0=442857.65 +a=6377298.556 +rf=300.8017"
SINU_W = "+proj=sinu +lon_0=10 +ellps=WGS84"
CEA_W = "+proj=cea +lat_ts=30 +lon_0=0 +ellps=WGS84"
ELLIPSOIDAL = [SINU_W, CEA_W, GEOS_MSG, GEOS_X, AEA_W, AEA_W1, LAEA_W, LAEA_WP, LAEA_WE, UTM33, UTM17S, ETMERC, TMERC_S, TMERC_B, STERE_W, STERE_WS, STERE_WP, STERE_WO, LCC_W, LCC_W1, MERC_W]

# the five pairs of the datum-shift tests: three and seven parameters, through projections
DATUM_PAIRS = [("+proj=latlong +datum=WGS84", "+proj=latlong +datum=potsdam"),
               ("+proj=latlong +datum=WGS84", "+proj=utm +zone=33 +ellps=intl +towgs84=-87,-98,-121"),                 # ED50
               ("+proj=latlong +ellps=bessel +towgs84=598.1,73.7,418.2,0.202,0.045,-2.455,6.7", "+proj=etmerc +lat_0=0 +lon_0=9 +k=1 +x_0=3500000 +datum=potsdam"),   # Gauss-Krueger zone 3
               ("+proj=latlong +datum=GGRS87", "+proj=stere +lat_0=90 +lon_0=0 +lat_ts=60 +datum=WGS84"),
               ("+proj=latlong +datum=WGS84", "+proj=latlong +datum=NAD83")]

UNIT_EXTRAS = ["+units=km", "+units=us-ft", "+to_meter=1/3.2808", "+pm=paris", "+pm=-17.5", "+units=km +pm=oslo", "+axis=enu +units=m"]

# strings the parser refuses (as the target of a transformation from GEO): the ones of test_unsupported_projection_strings_fail_loudly
UNSUPPORTED = ["+proj=utm +zone=33 +R=6371000", "+proj=utm +zone=0 +ellps=WGS84", "+proj=stere +lat_0=0 +ellps=WGS84", "+lat_0=3",
               "+proj=ob_tran +o_proj=stere +R=1", "+proj=ob_tran +o_proj=longlat +o_lat_p=30 +ellps=WGS84", "+proj=merc +ellps=WGS84 +units=parsec",
               "+proj=merc +R=6371000 +to_meter=0", "+proj=merc +R=6371000 +axis=wsu",
               "+proj=ob_tran +o_proj=longlat +o_lat_p=30 +R=6371000 +units=km", "+proj=merc +R=6371000 +pm=12d30",
               "+proj=merc +datum=NAD27", "+proj=merc +ellps=nonesuch", "+proj=stere +lat_0=90", "+proj=lcc +lat_1=30 +lat_2=-30 +R=1",
               "+proj=omerc +lat_0=60 +R=6371000", "+proj=ortho +lat_0=40 +ellps=WGS84", "+proj=nsper +lat_0=40 +R=6371000",
               "+proj=moll +R=6371000"]
NADGRIDS = "+proj=latlong +ellps=clrk66 +nadgrids=conus"   # grid shifts, from GEO_W
OMERC_TWO_POINT = "+proj=omerc +lat_0=40 +lat_1=47.5 +lon_1=-122.3 +lat_2=39 +lon_2=-104.5 +ellps=clrk66"


def is_degree(proj):
    return po.parse(proj)["proj"] in ("latlong", "longlat", "latlon", "lonlat", "ob_tran")


def close(a, b, proj):
    scale = 1.0 if is_degree(proj) else 6.4e6  # radians or metres
    np.testing.assert_allclose(a, b, rtol=0, atol=2e-13 * scale * 10)


def spherical_points(dst, n):
    """lon, lat (rad) of the round trip through a string of ALL, seeded by the string's length"""
    rng = np.random.default_rng(len(dst))
    lon = np.radians(rng.uniform(-60, 80, n))
    lat = np.radians(rng.uniform(-75 if dst in (STERE_S, MERC, STERE_EQ) else 20, 85 if dst != STERE_S else -30, n))
    return lon, lat


def ellipsoidal_points(dst, n):
    """lon, lat (rad) of the round trip through a string of ELLIPSOIDAL: transverse Mercator within 12 degrees of its meridian
    (Gauss-Krueger truncated; utm and etmerc carry the series to n^6 and hold far out), the satellite view on the visible disc"""
    rng = np.random.default_rng(len(dst))
    tm = "tmerc" in dst or "utm" in dst
    series = "proj=tmerc" in dst
    lon0 = np.degrees(po._Proj(dst).lam0)
    geos = "proj=geos" in dst
    lon = np.radians(rng.uniform(lon0 - 12, lon0 + 12, n) if series else (rng.uniform(lon0 - 40, lon0 + 40, n) if tm or geos else rng.uniform(-60, 80, n)))
    south = dst == STERE_WS
    lat = np.radians(rng.uniform(-85 if south else (-70 if tm or dst in (MERC_W, LAEA_WE) else 20), -30 if south else 85, n))
    if geos:
        lat = np.radians(rng.uniform(-60, 60, n))
    return lon, lat
