// The tile staging of the radius-1 stencil kernels (hdem_stencil.hip, hdem_terrain.hip); not
// part of the C ABI.  One 256-thread workgroup per 256 x 32 cell tile: the tile plus a
// one-cell halo is staged in LDS by coalesced 16-byte row loads, the halo columns sit at LDS
// columns 3 and 4+TW so that the interior stays 16-byte aligned for ds_read_b128, and a lane
// reads 6 consecutive values of one row (its 4 cells and their two neighbours).
#pragma once

#include "hdem_internal.h"

constexpr int TW = 256;          // tile width  (cells)
constexpr int TH = 32;           // tile height (cells), 4-byte elements
// 8-byte elements use half the rows so the tile stays under 64 KiB of LDS
template <typename T> struct tile_rows { static constexpr int value = sizeof(T) == 8 ? TH / 2 : TH; };
constexpr int LS = TW + 8;       // LDS row stride in elements, interior at col 4
constexpr int NT = 256;          // threads per workgroup

__device__ __forceinline__ int reflect(int i, int n)
{   // SciPy 'reflect': d c b a | a b c d | d c b a
    while (i < 0 || i >= n) {
        if (i < 0) i = -i - 1;
        if (i >= n) i = 2 * n - 1 - i;
    }
    return i;
}

// Stage rows y0-1..y0+TH, cols x0-1..x0+TW of `src` into `t`.
// REFLECT: out-of-raster cells mirror (box mean); otherwise they read the fill value: 0 (D8:
// only border cells see them and those are forced to code 0), or NaN with NANFILL (terrain
// attributes: one rule for the raster's edge and for nodata).
template <typename T, bool REFLECT, bool NANFILL = false>
__device__ __forceinline__ void stage_tile(const T *__restrict__ src, int H, int W,
                                           int y0, int x0, T *t)
{
    constexpr int THT = tile_rows<T>::value;
    constexpr int V = 16 / sizeof(T);            // elements per 16-byte load
    constexpr int CPR = TW / V;                  // chunks per row
    typedef T vec_t __attribute__((ext_vector_type(V)));
    typedef T vecu_t __attribute__((ext_vector_type(V), aligned(sizeof(T))));
    const T fill = NANFILL ? T(__builtin_nanf("")) : T(0);
    const int tid = threadIdx.x;
    // all of the thread's row chunks are requested before the first one is stored: a
    // load -> ds_write loop waits out one memory round trip per iteration
    constexpr int CHUNKS = ((THT + 2) * CPR + NT - 1) / NT;
    vec_t v[CHUNKS];
#pragma unroll
    for (int j = 0; j < CHUNKS; ++j) {
        const int i = tid + j * NT;
        const int r = i / CPR, c = (i % CPR) * V;
        int gy = y0 - 1 + r;
        const int gx = x0 + c;
        const bool row_ok = gy >= 0 && gy < H;
        if (REFLECT) gy = reflect(gy, H);
        if (i >= (THT + 2) * CPR) {
            v[j] = vec_t(T(0));
        } else if ((row_ok || REFLECT) && gx + V <= W) {
            v[j] = *reinterpret_cast<const vecu_t *>(src + (size_t)gy * W + gx);
        } else {
            for (int k = 0; k < V; ++k) {
                int xx = gx + k;
                T e = fill;
                if (REFLECT) e = src[(size_t)gy * W + reflect(xx, W)];
                else if (row_ok && xx < W) e = src[(size_t)gy * W + xx];
                v[j][k] = e;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < CHUNKS; ++j) {
        const int i = tid + j * NT;
        if (i < (THT + 2) * CPR)
            *reinterpret_cast<vec_t *>(t + (i / CPR) * LS + 4 + (i % CPR) * V) = v[j];
    }
    for (int i = tid; i < (THT + 2) * 2; i += NT) {
        int r = i >> 1, side = i & 1;
        int gy = y0 - 1 + r, gx = side ? x0 + TW : x0 - 1;
        T e = fill;
        if (REFLECT) e = src[(size_t)reflect(gy, H) * W + reflect(gx, W)];
        else if (gy >= 0 && gy < H && gx >= 0 && gx < W) e = src[(size_t)gy * W + gx];
        t[r * LS + (side ? 4 + TW : 3)] = e;
    }
}

// one LDS row -> 6 consecutive values (cols 4*cg-1 .. 4*cg+4 of the tile)
template <typename T>
__device__ __forceinline__ void read_row6(const T *t, int r, int cg, T (&o)[6])
{
    const T *p = t + r * LS + 4 + 4 * cg;
    o[0] = p[-1];
    o[1] = p[0]; o[2] = p[1]; o[3] = p[2]; o[4] = p[3];
    o[5] = p[4];
}
