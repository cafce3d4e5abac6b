// Depression labelling and inventory (new operator; Depressions, DepressionInventory).
//
// raised(c) = filled[c] > dem[c] (false when either is NaN).  A depression is an 8-connected
// component of raised cells, first(D) its smallest flat index y * W + x.
//   first mode    label[c] = 1 + first(D), 0 where c is not raised
//   compact mode  the depressions numbered 1 ... K in ascending order of first: the numbering
//                 of scipy.ndimage.label with the 3 x 3 structure
// The tiles are those of hdem_d8tile.h (64 x 64, one workgroup per tile); nothing else of the
// D8 forest is used: that one follows one pointer per cell downstream, this one groups cells
// by adjacency.  The label raster is its own union-find forest, parent(c) = out[c] - 1 with
// every pointer going to a smaller index, so there is no per-cell workspace for the labelling
// and no cycle to fall into.
//   A   (depr_tile_kernel)    per tile: the raised mask as 64 row words in LDS, every cell
//       labelled with the start of its row run, then rounds of "hang my root under the
//       smallest root one of my 8 neighbours has" (LDS atomicMin) + full path compression
//       until a round changes nothing.  A link the atomicMin overwrites is found again by the
//       next round's scan; at the fixed point all cells of a component share one root, the
//       smallest local index, which is also the smallest flat index (both row-major).
//   B   (depr_seam_kernel)    one thread per cell along a tile seam: the lock-free union of
//       the roots of the (up to three) raised cells it faces, the larger root hung under the
//       smaller with atomicMin.  A pair is skipped when the labels show that a neighbouring
//       pair along the seam joins the same two tile components.  Only words of tile roots
//       are written; the root of a component ends as the minimum of its tile roots: first(D).
//   C1  (depr_roots_kernel)   the tile perimeters only: every tile root that was hung is the
//       label of a perimeter cell of its tile; each is pointed straight at its true root.
//   C2  (depr_final_kernel)   streaming: label -> tile root -> root.  Only true roots are
//       written and roots do not change in C, so whatever a racing reader sees is an ancestor.
//       Compact mode: also one bit per cell "is a root" and the count per 64-cell word.
//   N   (hdem_scan.h / depr_relabel_kernel)  compact mode: the shared exclusive scan of the word
//       counts (chunk sums, one workgroup over the sums, apply), then rank of a root = scanned
//       count of its word + popcount of the bits in front of it; label = 1 + rank of the
//       cell's root.
// Table (hdem_depression_table_f32): one pass over dem, filled and compact labels; a
// workgroup gathers its tile per label in an LDS hash table (a tile holds at most 1 024
// components, the table has 1 024 slots), then one global atomic per (tile, label, column).
// Every column is a min, a max or an integer sum: bit-reproducible.
// Every find, union and propagation loop has an explicit cap; running into one is counted and
// reported as HDEM_ERR_NOT_CONVERGED.  No workgroup waits for another.
// Workspace (arena): compact mode 12 B per 64 cells (bitmap + counts); first mode and the
// table 512 B.
#include "hdem_d8tile.h"
#include "hdem_scan.h"

namespace {

constexpr int NT = 256;               // threads of the seam, roots, final and table workgroups
constexpr int ANT = 512;              // threads of the tile workgroup (8 rows per pass)
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr int SLOTS = 1024;           // hash slots of the table kernel: >= components per tile
constexpr size_t HEAD = 512;          // bytes of the counter block in front of the arena

struct depr_counters {
    unsigned long long raised;        // raised cells
    unsigned long long tile_components;   // components of phase A, summed over the tiles
    unsigned long long roots;         // K
    unsigned long long capped;        // loops that ran into their cap
    unsigned long long bad_label;     // table: labels > K
    unsigned long long foreign;       // table: labelled cells that are not raised
};
static_assert(sizeof(depr_counters) <= HEAD, "counters outgrew their block");

// words of the forest are written by other workgroups during B and C1
__device__ __forceinline__ uint32_t word_load(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void word_store(uint32_t *p, uint32_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ bool is_raised(float z, float w) { return w > z; }

// A.
__global__ __launch_bounds__(ANT) void depr_tile_kernel(const float *__restrict__ dem,
                                                        const float *__restrict__ filled, int H,
                                                        int W, int tiles_x, uint32_t *out,
                                                        depr_counters *__restrict__ cnt)
{
    __shared__ unsigned long long rows[TS + 2];  // raised mask of row ly in rows[ly + 1]
    __shared__ uint32_t lab[TC];                 // parent (local index) of a raised cell
    __shared__ unsigned int s_cnt[3];            // raised, components, capped

    const int tid = threadIdx.x;
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    if (tid < 3) s_cnt[tid] = 0;
    if (tid == 0) rows[0] = rows[TS + 1] = 0;
    __syncthreads();

    // a wave is a row of the tile: the mask by ballot, the label the start of the cell's run
    unsigned int raised = 0;
    for (int i = tid; i < TC; i += ANT) {
        const int ly = i / TS, lx = i % TS;
        bool r = false;
        if (tile.inside(ly, lx)) {
            const size_t g = (size_t)(tile.y0 + ly) * W + tile.x0 + lx;
            r = is_raised(dem[g], filled[g]);
        }
        const unsigned long long m = __ballot(r);
        if (lx == 0) rows[ly + 1] = m;
        const unsigned long long gaps = ~m & ((1ull << lx) - 1);     // unraised cells before lx
        const int start = gaps ? 64 - __builtin_clzll(gaps) : 0;
        lab[i] = r ? (uint32_t)(ly * TS + start) : NONE;
        raised += r;
    }
    if (raised) atomicAdd(&s_cnt[0], raised);
    __syncthreads();

    // Labels only decrease and a round that changes something removes a root, so TC rounds
    // bound the loop.  (How many a tile takes has not been counted; the spiral corridor
    // costs the time of a full square.)
    unsigned int capped = 0;
    int round = 0;
    for (; round < TC; ++round) {
        int changed = 0;
        for (int i = tid; i < TC; i += ANT) {
            const int ly = i / TS, lx = i % TS;
            if (!((rows[ly + 1] >> lx) & 1)) continue;
            const uint32_t mine = lab[i];
            uint32_t least = mine;
            for (int dy = -1; dy <= 1; ++dy) {
                const unsigned long long m = rows[ly + 1 + dy];
                for (int dx = -1; dx <= 1; ++dx) {
                    const int nx = lx + dx;
                    if (nx < 0 || nx >= TS || !((m >> nx) & 1)) continue;
                    least = min(least, lab[(ly + dy) * TS + nx]);
                }
            }
            if (least < mine) {
                atomicMin(&lab[mine], least);
                changed = 1;
            }
        }
        if (!__syncthreads_or(changed)) break;
        // every cell to its root; whatever a racing reader sees is an ancestor
        for (int i = tid; i < TC; i += ANT) {
            const int ly = i / TS, lx = i % TS;
            if (!((rows[ly + 1] >> lx) & 1)) continue;
            uint32_t r = lab[i], p = lab[r];
            for (int step = 0; p != r && step < TC; ++step) {
                r = p;
                p = lab[r];
            }
            capped += p != r;
            lab[i] = r;
        }
        __syncthreads();
    }
    capped += round == TC && tid == 0;

    unsigned int comps = 0;
    for (int i = tid; i < TC; i += ANT) {
        const int ly = i / TS, lx = i % TS;
        if (!tile.inside(ly, lx)) continue;
        const size_t g = (size_t)(tile.y0 + ly) * W + tile.x0 + lx;
        const uint32_t r = lab[i];
        comps += r == (uint32_t)i;
        out[g] = r == NONE ? 0u
                           : (uint32_t)((size_t)(tile.y0 + r / TS) * W + tile.x0 + r % TS) + 1u;
    }
    if (comps) atomicAdd(&s_cnt[1], comps);
    if (capped) atomicAdd(&s_cnt[2], capped);
    __syncthreads();
    if (tid == 0) {
        if (s_cnt[0]) atomicAdd(&cnt->raised, (unsigned long long)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&cnt->tile_components, (unsigned long long)s_cnt[1]);
        if (s_cnt[2]) atomicAdd(&cnt->capped, (unsigned long long)s_cnt[2]);
    }
}

// The root of label l (1 + index), halving the path behind it: a word is only ever lowered to
// an ancestor's label.  `cap` bounds the chain: it holds tile roots only.
__device__ __forceinline__ uint32_t find_halving(uint32_t *out, uint32_t l, uint32_t cap,
                                                 unsigned int &capped)
{
    uint32_t p = word_load(&out[l - 1]);
    uint32_t step = 0;
    while (p != l && step++ < cap) {
        const uint32_t gp = word_load(&out[p - 1]);
        if (gp != p) atomicMin(&out[l - 1], gp);
        l = p;
        p = gp;
    }
    capped += p != l;
    return l;
}

// The textbook lock-free union: the larger root under the smaller.  What the atomic returns
// is what is trusted; the larger of the two labels strictly decreases with every turn.
__device__ __forceinline__ void unite(uint32_t *out, uint32_t a, uint32_t b, uint32_t cap,
                                      unsigned int &capped)
{
    a = find_halving(out, a, cap, capped);
    b = find_halving(out, b, cap, capped);
    uint32_t step = 0;
    while (a != b && step++ < cap) {
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        const uint32_t old = atomicMin(&out[a - 1], b);
        if (old == a) return;
        a = old;
    }
    capped += a != b;
}

// B.  Items: for every vertical seam the H cells left of it, then for every horizontal seam
// the W cells above it.  Cell a = item, b[-1 .. 1] the three cells it faces across the seam,
// counted along the seam.  With la / lb the labels along the seam:
//   straight (a, b0)     skipped when the pair before it has the same two labels
//   diagonal (a, b+-1)   skipped when b+-1 has b0's label (the straight pair does it) or
//                        a+-1 has a's label (that cell's straight pair does it)
// Equal labels mean a common ancestor, so every skip leaves the join to a pair that is made.
__global__ __launch_bounds__(NT) void depr_seam_kernel(int H, int W, int tiles_x, int tiles_y,
                                                       uint32_t *out,
                                                       depr_counters *__restrict__ cnt)
{
    const int64_t nv = (int64_t)(tiles_x - 1) * H, nh = (int64_t)(tiles_y - 1) * W;
    const int64_t item = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (item >= nv + nh) return;
    // a chain holds tile roots only (A's count is final: it was a launch of its own)
    const unsigned long long comps = cnt->tile_components;
    const uint32_t cap = comps >= 0xFFFFFFFEull ? 0xFFFFFFFFu : (uint32_t)comps + 1u;

    int64_t a0, b0, along;            // flat index of a and of b0, the step along the seam
    int pos, len;
    if (item < nv) {
        const int x = (int)(item / H + 1) * TS;
        pos = (int)(item % H), len = H, along = W;
        a0 = (int64_t)pos * W + x - 1, b0 = a0 + 1;
    } else {
        const int64_t k = item - nv;
        const int y = (int)(k / W + 1) * TS;
        pos = (int)(k % W), len = W, along = 1;
        a0 = (int64_t)(y - 1) * W + pos, b0 = a0 + W;
    }
    const uint32_t la = word_load(&out[a0]);
    if (!la) return;
    const bool before = pos > 0, after = pos + 1 < len;
    const uint32_t lb = word_load(&out[b0]);
    const uint32_t la_m = before ? word_load(&out[a0 - along]) : 0u;
    const uint32_t lb_m = before ? word_load(&out[b0 - along]) : 0u;
    const uint32_t la_p = after ? word_load(&out[a0 + along]) : 0u;
    const uint32_t lb_p = after ? word_load(&out[b0 + along]) : 0u;

    unsigned int capped = 0;
    if (lb && !(la_m == la && lb_m == lb)) unite(out, la, lb, cap, capped);
    if (lb_m && lb_m != lb && la_m != la) unite(out, la, lb_m, cap, capped);
    if (lb_p && lb_p != lb && la_p != la) unite(out, la, lb_p, cap, capped);
    if (capped) atomicAdd(&cnt->capped, (unsigned long long)capped);
}

// The root of label l without writing; roots are stable in C.
__device__ __forceinline__ uint32_t find_root(const uint32_t *out, uint32_t l, uint32_t cap,
                                              unsigned int &capped)
{
    uint32_t p = word_load(&out[l - 1]);
    uint32_t step = 0;
    while (p != l && step++ < cap) {
        l = p;
        p = word_load(&out[l - 1]);
    }
    capped += p != l;
    return l;
}

// C1: the perimeter cells.  The label of one is a tile root (or, where the cell is a tile root
// itself, already an ancestor); that root and every node on its chain get the true root.
__global__ __launch_bounds__(NT) void depr_roots_kernel(int H, int W, int tiles_x, uint32_t *out,
                                                        depr_counters *__restrict__ cnt)
{
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    const int tid = threadIdx.x;
    if (tid >= PER) return;
    int ly, lx;
    perim_cell(tid, ly, lx);
    if (!tile.inside(ly, lx)) return;
    const unsigned long long comps = cnt->tile_components;
    const uint32_t cap = comps >= 0xFFFFFFFEull ? 0xFFFFFFFFu : (uint32_t)comps + 1u;
    const size_t g = (size_t)(tile.y0 + ly) * W + tile.x0 + lx;
    uint32_t l = out[g];
    if (!l) return;
    // the cell before on the same side shares the label more often than not: its thread
    // does the work (a perimeter cell's own word changes only when its chain is done)
    if (tid < 2 * TS ? lx > 0 && word_load(&out[g - 1]) == l : word_load(&out[g - W]) == l)
        return;
    unsigned int capped = 0;
    const uint32_t root = find_root(out, l, cap, capped);
    uint32_t step = 0;
    while (l != root && step++ < cap) {
        const uint32_t next = word_load(&out[l - 1]);
        if (next != root) word_store(&out[l - 1], root);
        l = next;
    }
    if (capped) atomicAdd(&cnt->capped, (unsigned long long)capped);
}

// C2.  COMPACT: also bits[y * tiles_x + tx] = which cells of the word are roots, and their count.
template <bool COMPACT>
__global__ __launch_bounds__(NT) void depr_final_kernel(int H, int W, int tiles_x, uint32_t *out,
                                                        unsigned long long *__restrict__ bits,
                                                        uint32_t *__restrict__ count,
                                                        depr_counters *__restrict__ cnt)
{
    __shared__ unsigned int s_cnt[2];            // roots, capped
    const int tid = threadIdx.x;
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();

    unsigned int roots = 0, capped = 0;
    for (int i = tid; i < TC; i += NT) {
        const int ly = i / TS, lx = i % TS;
        if (ly >= tile.th) break;                // (whole waves: a wave is a row)
        bool root = false;
        if (lx < tile.tw) {
            const size_t g = (size_t)(tile.y0 + ly) * W + tile.x0 + lx;
            const uint32_t l = out[g];
            if (l) {
                // label -> tile root -> root: two hops after C1, three where a hung tile
                // root is the one perimeter cell with its label (C1 started from that cell's
                // word, its old parent); the cap is for a wrong build
                const uint32_t r = find_root(out, l, 64u, capped);
                if (r != l) out[g] = r;
                root = r == (uint32_t)g + 1u;
            }
        }
        if (COMPACT) {
            const unsigned long long m = __ballot(root);
            if (lx == 0) {
                const size_t w = (size_t)(tile.y0 + ly) * tiles_x + tile.tx;
                bits[w] = m;
                count[w] = (uint32_t)__popcll(m);
            }
        }
        roots += root;
    }
    if (roots) atomicAdd(&s_cnt[0], roots);
    if (capped) atomicAdd(&s_cnt[1], capped);
    __syncthreads();
    if (tid == 0) {
        if (s_cnt[0]) atomicAdd(&cnt->roots, (unsigned long long)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&cnt->capped, (unsigned long long)s_cnt[1]);
    }
}

// label 1 + first -> 1 + rank of that root.  A thread reads no label but its own cell's.
__global__ __launch_bounds__(NT) void depr_relabel_kernel(int64_t cells, int W, int tiles_x,
                                                          const unsigned long long *__restrict__ bits,
                                                          const uint32_t *__restrict__ before,
                                                          uint32_t *__restrict__ out)
{
    for (int64_t c = (int64_t)blockIdx.x * NT + threadIdx.x; c < cells;
         c += (int64_t)gridDim.x * NT) {
        const uint32_t l = out[c];
        if (!l) continue;
        const uint32_t r = l - 1u;
        const uint32_t ry = r / (uint32_t)W, rx = r - ry * (uint32_t)W;
        const size_t w = (size_t)ry * tiles_x + rx / TS;
        out[c] = 1u + hdem_rank_in(bits[w], (int)(rx % TS), before[w]);
    }
}

// ---------------------------------------------------------------------------
// the table
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void depr_table_init_kernel(int64_t K, uint32_t *first,
                                                             uint32_t *area, uint32_t *level,
                                                             uint32_t *depth,
                                                             unsigned long long *volume)
{
    const int64_t k = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (k >= K) return;
    if (first) first[k] = 0xFFFFFFFFu;
    if (area) area[k] = 0u;
    if (level) level[k] = 0xFFFFFFFFu;
    if (depth) depth[k] = 0u;
    if (volume) volume[k] = 0ull;
}

__global__ __launch_bounds__(NT) void depr_table_level_kernel(int64_t K, uint32_t *level)
{
    const int64_t k = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (k < K) level[k] = __float_as_uint(float_of(level[k]));
}

struct depr_row {                     // what one cell, or one wave of one label, adds to a row
    uint32_t label, area, first, level, depth;
    unsigned long long volume;
};

__global__ __launch_bounds__(NT) void depr_table_kernel(
    const float *__restrict__ dem, const float *__restrict__ filled,
    const uint32_t *__restrict__ labels, int H, int W, int tiles_x, int64_t K, uint32_t *first,
    uint32_t *area, uint32_t *level, uint32_t *depth, unsigned long long *volume,
    depr_counters *__restrict__ cnt)
{
    __shared__ uint32_t s_key[SLOTS], s_area[SLOTS], s_first[SLOTS], s_level[SLOTS],
        s_depth[SLOTS];
    __shared__ unsigned long long s_volume[SLOTS];
    __shared__ unsigned int s_cnt[3];            // labels > K, foreign cells, capped

    const int tid = threadIdx.x;
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    for (int s = tid; s < SLOTS; s += NT) {
        s_key[s] = 0u, s_area[s] = 0u, s_first[s] = 0xFFFFFFFFu, s_level[s] = 0xFFFFFFFFu;
        s_depth[s] = 0u, s_volume[s] = 0ull;
    }
    if (tid < 3) s_cnt[tid] = 0;
    __syncthreads();

    unsigned int bad = 0, foreign = 0, capped = 0;
    for (int i = tid; i < TC; i += NT) {
        const int ly = i / TS, lx = i % TS;
        if (ly >= tile.th) break;                // (whole waves: a wave is a row)
        depr_row row = {0u, 1u, 0u, 0u, 0u, 0ull};
        if (lx < tile.tw) {
            const size_t g = (size_t)(tile.y0 + ly) * W + tile.x0 + lx;
            const uint32_t l = labels[g];
            if (l) {
                const float z = dem[g], w = filled[g];
                if ((int64_t)l > K) {
                    ++bad;
                } else if (!is_raised(z, w)) {
                    ++foreign;
                } else {
                    const float d = w - z;       // > 0
                    const double q = rint((double)d * 1048576.0);
                    row.label = l;
                    row.first = (uint32_t)g;
                    row.level = key_of(w);
                    row.depth = __float_as_uint(d);
                    row.volume = q >= 2147483647.0 ? 2147483647ull : (unsigned long long)q;
                }
            }
        }
        // A row of one lake (or of none) is one wave with one label: reduce in the wave.
        // Every wave-wide operation of an iteration comes before its lanes part: the
        // inserts below are the last thing in the loop body and nothing leaves it early.
        const uint32_t l0 = __builtin_amdgcn_readfirstlane(row.label);
        const bool uniform = __all(row.label == l0);
        bool insert = row.label != 0u;
        if (uniform && l0) {
            for (int m = 32; m >= 1; m >>= 1) {
                row.area += __shfl_xor(row.area, m);
                row.first = min(row.first, (uint32_t)__shfl_xor(row.first, m));
                row.level = min(row.level, (uint32_t)__shfl_xor(row.level, m));
                row.depth = max(row.depth, (uint32_t)__shfl_xor(row.depth, m));
                row.volume += __shfl_xor(row.volume, m);
            }
            insert = lx == 0;
        }
        if (insert) {
            uint32_t s = (row.label * 2654435761u) >> 22;        // 10 bits
            int probe = 0;
            for (; probe < SLOTS; ++probe) {
                const uint32_t seen = atomicCAS(&s_key[s], 0u, row.label);
                if (seen == 0u || seen == row.label) break;
                s = (s + 1) & (SLOTS - 1);
            }
            if (probe < SLOTS) {
                atomicAdd(&s_area[s], row.area);
                atomicMin(&s_first[s], row.first);
                atomicMin(&s_level[s], row.level);
                atomicMax(&s_depth[s], row.depth);
                atomicAdd(&s_volume[s], row.volume);
            } else {                             // more than 1 024 labels in a tile: not from A
                ++capped;
            }
        }
    }
    if (bad) atomicAdd(&s_cnt[0], bad);
    if (foreign) atomicAdd(&s_cnt[1], foreign);
    if (capped) atomicAdd(&s_cnt[2], capped);
    __syncthreads();

    // one global atomic per (tile, label) and column
    for (int s = tid; s < SLOTS; s += NT) {
        const uint32_t l = s_key[s];
        if (!l) continue;
        const size_t k = l - 1u;                 // l <= K was checked on the way in
        if (area) atomicAdd(&area[k], s_area[s]);
        if (first) atomicMin(&first[k], s_first[s]);
        if (level) atomicMin(&level[k], s_level[s]);
        if (depth) atomicMax(&depth[k], s_depth[s]);
        if (volume) atomicAdd(&volume[k], s_volume[s]);
    }
    if (tid == 0) {
        if (s_cnt[0]) atomicAdd(&cnt->bad_label, (unsigned long long)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&cnt->foreign, (unsigned long long)s_cnt[1]);
        if (s_cnt[2]) atomicAdd(&cnt->capped, (unsigned long long)s_cnt[2]);
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// also the tile grid: nothing is allocated for a raster that is refused
int check_label_args(hdem_ctx *ctx, const float *dem, const float *filled, int H, int W, int flags,
                     uint32_t *labels, hdem_depressions_stats *stats, d8_grid *g)
{
    if (int rc = hdem_check_call(ctx, dem, labels, H, W)) return rc;
    HDEM_REQUIRE(filled, HDEM_ERR_BAD_ARG, "null raster pointer");
    if (int rc = d8_grid_of("depression labelling", H, W, g)) return rc;
    HDEM_REQUIRE(!(flags & ~HDEM_DEPR_COMPACT), HDEM_ERR_BAD_ARG, "unknown depression flags 0x%x",
                 flags);
    return d8_check_stats(stats, "hdem_depressions_stats");
}

int check_table_args(hdem_ctx *ctx, const float *dem, const float *filled, const uint32_t *labels,
                     int H, int W, int64_t K, const void *first, const void *area,
                     const void *level, const void *max_depth, const void *volume_q20, d8_grid *g)
{
    if (int rc = hdem_check_call(ctx, dem, filled, H, W)) return rc;
    HDEM_REQUIRE(labels, HDEM_ERR_BAD_ARG, "null raster pointer");
    if (int rc = d8_grid_of("the depression table", H, W, g)) return rc;
    HDEM_REQUIRE(K >= 0 && K <= (int64_t)H * W, HDEM_ERR_BAD_ARG,
                 "K is the number of depressions, 0 ... H * W: got %lld", (long long)K);
    HDEM_REQUIRE(first || area || level || max_depth || volume_q20, HDEM_ERR_BAD_ARG,
                 "no column wanted: at least one of first, area, level, max_depth and "
                 "volume_q20 must not be null");
    return HDEM_OK;
}

int report_capped(unsigned long long capped)
{
    HDEM_REQUIRE(!capped, HDEM_ERR_NOT_CONVERGED,
                 "depression labelling: %llu loops ran into their iteration cap", capped);
    return HDEM_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int hdem_depressions_f32_dev(hdem_ctx *ctx, const float *dem, const float *filled,
                                        int H, int W, int flags, uint32_t *labels,
                                        hdem_depressions_stats *stats)
{
    d8_grid g;
    if (int rc = check_label_args(ctx, dem, filled, H, W, flags, labels, stats, &g)) return rc;
    const bool compact = (flags & HDEM_DEPR_COMPACT) != 0;
    const int64_t cells = (int64_t)H * W;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    hdem_depressions_stats st = {};
    d8_publish(stats, st);

    // arena: counters | the rank table of the root bits (compact mode)
    const int64_t words = compact ? (int64_t)H * g.tiles_x : 0;
    char *ws = static_cast<char *>(hdem_arena(ctx, HEAD + hdem_rank_table_bytes(words)));
    if (!ws) return HDEM_ERR_OOM;
    depr_counters *cnt = reinterpret_cast<depr_counters *>(ws);
    hdem_rank_table rank;
    hdem_rank_table_at(ws + HEAD, words, &rank);

    hdem_event_timer<4> phases(ctx, stats != nullptr);
    if (int rc = phases.start()) return rc;

    HDEM_HIP_CHECK(hipMemsetAsync(cnt, 0, HEAD, ctx->stream));
    const dim3 grid((unsigned)g.tiles);
    const int64_t seam_items = (int64_t)(g.tiles_x - 1) * H + (int64_t)(g.tiles_y - 1) * W;

    phases.mark(0);
    hipLaunchKernelGGL(depr_tile_kernel, grid, dim3(ANT), 0, ctx->stream, dem, filled, H, W,
                       g.tiles_x, labels, cnt);
    phases.mark(1);
    if (seam_items)
        hipLaunchKernelGGL(depr_seam_kernel, dim3((unsigned)((seam_items + NT - 1) / NT)),
                           dim3(NT), 0, ctx->stream, H, W, g.tiles_x, g.tiles_y, labels, cnt);
    phases.mark(2);
    if (seam_items)
        hipLaunchKernelGGL(depr_roots_kernel, grid, dim3(NT), 0, ctx->stream, H, W, g.tiles_x,
                           labels, cnt);
    if (compact) {
        hipLaunchKernelGGL(depr_final_kernel<true>, grid, dim3(NT), 0, ctx->stream, H, W,
                           g.tiles_x, labels, rank.bits, rank.count, cnt);
        hdem_scan_exclusive(ctx->stream, rank.count, words, rank.sums);
        const int relabel_grid =
            (int)std::min<int64_t>((cells + NT - 1) / NT, (int64_t)ctx->num_cus * 8);
        hipLaunchKernelGGL(depr_relabel_kernel, dim3(relabel_grid), dim3(NT), 0, ctx->stream,
                           cells, W, g.tiles_x, rank.bits, rank.count, labels);
    } else {
        hipLaunchKernelGGL(depr_final_kernel<false>, grid, dim3(NT), 0, ctx->stream, H, W,
                           g.tiles_x, labels, rank.bits, rank.count, cnt);
    }
    phases.mark(3);
    HDEM_HIP_CHECK(hipGetLastError());
    depr_counters host = {};
    HDEM_HIP_CHECK(hipMemcpyAsync(&host, cnt, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
    HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));

    st.depressions = (int64_t)host.roots;
    st.raised_cells = (int64_t)host.raised;
    st.tile_components = (int64_t)host.tile_components;
    st.tile_h = TS;
    st.tile_w = TS;
    phases.read(&st.ms_tile, &st.ms_seam, &st.ms_final);
    d8_publish(stats, st);
    return report_capped(host.capped);
}

extern "C" int hdem_depressions_f32(hdem_ctx *ctx, const float *dem, const float *filled, int H,
                                    int W, int flags, uint32_t *labels,
                                    hdem_depressions_stats *stats)
{
    d8_grid g;
    if (int rc = check_label_args(ctx, dem, filled, H, W, flags, labels, stats, &g)) return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)H * W * 4;
    hdem_dbuf ddem, dfilled, dlabels;
    if (int rc = ddem.upload(ctx, dem, bytes)) return rc;
    if (int rc = dfilled.upload(ctx, filled, bytes)) return rc;
    if (int rc = dlabels.alloc(ctx, bytes)) return rc;
    if (int rc = hdem_depressions_f32_dev(ctx, ddem.as<const float>(), dfilled.as<const float>(),
                                          H, W, flags, dlabels.as<uint32_t>(), stats))
        return rc;
    return dlabels.download(labels, bytes);
}

extern "C" int hdem_depression_table_f32_dev(hdem_ctx *ctx, const float *dem, const float *filled,
                                             const uint32_t *labels, int H, int W, int64_t K,
                                             uint32_t *first, uint32_t *area, float *level,
                                             float *max_depth, uint64_t *volume_q20)
{
    d8_grid g;
    if (int rc = check_table_args(ctx, dem, filled, labels, H, W, K, first, area, level, max_depth,
                                  volume_q20, &g))
        return rc;
    if (K == 0) return HDEM_OK;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    depr_counters *cnt = static_cast<depr_counters *>(hdem_arena(ctx, HEAD));
    if (!cnt) return HDEM_ERR_OOM;
    HDEM_HIP_CHECK(hipMemsetAsync(cnt, 0, HEAD, ctx->stream));
    // level is gathered as an order-preserving key, max_depth as the bits of a positive float
    uint32_t *level_key = reinterpret_cast<uint32_t *>(level);
    uint32_t *depth_bits = reinterpret_cast<uint32_t *>(max_depth);
    unsigned long long *volume = reinterpret_cast<unsigned long long *>(volume_q20);
    const dim3 rows((unsigned)((K + NT - 1) / NT));
    hipLaunchKernelGGL(depr_table_init_kernel, rows, dim3(NT), 0, ctx->stream, K, first, area,
                       level_key, depth_bits, volume);
    hipLaunchKernelGGL(depr_table_kernel, dim3((unsigned)g.tiles), dim3(NT), 0, ctx->stream, dem,
                       filled, labels, H, W, g.tiles_x, K, first, area, level_key, depth_bits,
                       volume, cnt);
    if (level)
        hipLaunchKernelGGL(depr_table_level_kernel, rows, dim3(NT), 0, ctx->stream, K, level_key);
    HDEM_HIP_CHECK(hipGetLastError());
    depr_counters host = {};
    HDEM_HIP_CHECK(hipMemcpyAsync(&host, cnt, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
    HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    HDEM_REQUIRE(!host.bad_label, HDEM_ERR_BAD_ARG,
                 "%llu cells hold a label greater than K = %lld", host.bad_label, (long long)K);
    HDEM_REQUIRE(!host.foreign, HDEM_ERR_BAD_ARG,
                 "the labels do not belong to these rasters: %llu cells are labelled and not "
                 "raised",
                 host.foreign);
    return report_capped(host.capped);
}

extern "C" int hdem_depression_table_f32(hdem_ctx *ctx, const float *dem, const float *filled,
                                         const uint32_t *labels, int H, int W, int64_t K,
                                         uint32_t *first, uint32_t *area, float *level,
                                         float *max_depth, uint64_t *volume_q20)
{
    d8_grid g;
    if (int rc = check_table_args(ctx, dem, filled, labels, H, W, K, first, area, level, max_depth,
                                  volume_q20, &g))
        return rc;
    if (K == 0) return HDEM_OK;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)H * W * 4, n = (size_t)K;
    hdem_dbuf ddem, dfilled, dlabels, dfirst, darea, dlevel, ddepth, dvolume;
    if (int rc = ddem.upload(ctx, dem, bytes)) return rc;
    if (int rc = dfilled.upload(ctx, filled, bytes)) return rc;
    if (int rc = dlabels.upload(ctx, labels, bytes)) return rc;
    struct column {
        hdem_dbuf *dev;
        void *host;
        size_t bytes;
    } columns[] = {{&dfirst, first, n * 4}, {&darea, area, n * 4}, {&dlevel, level, n * 4},
                   {&ddepth, max_depth, n * 4}, {&dvolume, volume_q20, n * 8}};
    for (column &c : columns)
        if (c.host)
            if (int rc = c.dev->alloc(ctx, c.bytes)) return rc;
    if (int rc = hdem_depression_table_f32_dev(
            ctx, ddem.as<const float>(), dfilled.as<const float>(), dlabels.as<const uint32_t>(),
            H, W, K, dfirst.as<uint32_t>(), darea.as<uint32_t>(), dlevel.as<float>(),
            ddepth.as<float>(), dvolume.as<uint64_t>()))
        return rc;
    for (column &c : columns)
        if (c.host)
            if (int rc = c.dev->download(c.host, c.bytes)) return rc;
    return HDEM_OK;
}
