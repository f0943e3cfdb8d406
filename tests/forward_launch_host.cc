// C entry point over fimex_amd/csrc/forward_launch.hpp for the CPU: tests/forward_launch_host.py compiles this file with g++ into a
// temporary directory and calls it through ctypes.
#include "forward_launch.hpp"

using namespace fimex_amd::forward_launch;

extern "C" {

// in[6]: nOut, nz, mappedSourceCells, undefinedCells, maxBucket, aggregate; tuning[7] in the order of Tuning's members (-1: not set);
// out[9]: family, zc, ahead, rank, rankAll, zPerBlock, chunks, laneGridX, chunksFit
void fl_forward_launch(const uint64_t* in, int tilesValid, const int* tuning, uint64_t* out, double* meanBucket)
{
    Tuning t;
    t.tiled = tuning[0];
    t.zpb = tuning[1];
    t.wave = tuning[2];
    t.medianShort = tuning[3];
    t.medianWaveMin = tuning[4];
    t.medianWave = tuning[5];
    t.medianZc = tuning[6];
    const Launch l = forward_launch(in[0], in[1], in[2], in[3], in[4], (int)in[5], tilesValid != 0, t);
    out[0] = (uint64_t)l.family;
    out[1] = (uint64_t)l.zc;
    out[2] = (uint64_t)l.ahead;
    out[3] = l.rank ? 1 : 0;
    out[4] = l.rankAll ? 1 : 0;
    out[5] = l.zPerBlock;
    out[6] = l.chunks;
    out[7] = l.laneGridX;
    out[8] = l.chunksFit() ? 1 : 0;
    *meanBucket = l.meanBucket;
}

}  // extern "C"
