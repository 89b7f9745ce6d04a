// rdm_plan_check.cpp — the host-side plan of the density matrices (openvqe_amd/csrc/sv_rdm_host.hpp) compiled alone with g++ (ASan +
// UBSan: tests/test_rdm_host.py).  Checks, for n = 1..9 and states of several densities:
//   - the column tables (added bits, between masks) against their definition orbital by orbital
//   - shadow_word() over partial-word, one-word and multi-word bitmaps against the brute-force down-shadow
//   - the row list (set bits of the shadow, word by word from the popcount prefix sums): ascending and complete
//   - the schedule: every (row, block pair) belongs to exactly one (chunk, slice, tile) and the owned columns tile a block
//   - a replay of k_rdm_rows + k_rdm_gram + k_rdm_finish with the kernels' indexing (workspace chunks, staged 16-byte units, 256 threads
//     with 4 x 4 accumulators, slabs per (block pair, slice) summed in slice order) against the definition, to 1e-13
//   - the schedules of the cases A - F of tests/test_gpu_rdm_edges.py at 256 compute units: the cover of every chunk by (pair, slice,
//     tile), the empty slices of the last launch, the trips of the grid-stride loops; block_pair / block_pair_index for 1 - 7 blocks
//   usage: rdm_plan_check [seed]
#include "../../openvqe_amd/csrc/sv_rdm_host.hpp"

#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

using namespace ovqe;
typedef std::complex<double> cplx;

static int g_fail = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");                \
            if (++g_fail > 20) std::exit(1);  \
        }                                     \
    } while (0)

static int occ_between(uint64_t K, int n, int lo, int hi) {   // occupied orbitals t with lo < t < hi
    int c = 0;
    for (int t = lo + 1; t < hi; ++t) c += (int)((K >> (n - 1 - t)) & 1);
    return c;
}

static void check_columns(int n) {
    std::vector<rdm::ColEntry> c1, c2;
    rdm::build_columns(n, 1, c1);
    CHECK((int64_t)c1.size() == rdm::width(n, 1), "order-1 width n=%d", n);
    for (int a = 0; a < n; ++a) {
        CHECK(c1[a].add == (1ull << (n - 1 - a)), "order-1 add n=%d a=%d", n, a);
        for (uint64_t K = 0; K < (1ull << n); ++K)
            CHECK((__builtin_popcountll(K & c1[a].between) & 1) == (occ_between(K, n, -1, a) & 1), "order-1 sign n=%d a=%d", n, a);
    }
    if (n < 2) return;
    rdm::build_columns(n, 2, c2);
    CHECK((int64_t)c2.size() == rdm::width(n, 2), "order-2 width n=%d", n);
    size_t at = 0;
    for (int a = 0; a < n; ++a)
        for (int b = a + 1; b < n; ++b, ++at) {
            CHECK(c2[at].add == ((1ull << (n - 1 - a)) | (1ull << (n - 1 - b))), "order-2 add n=%d (%d,%d)", n, a, b);
            for (uint64_t K = 0; K < (1ull << n); ++K)
                CHECK((__builtin_popcountll(K & c2[at].between) & 1) == (occ_between(K, n, a, b) & 1), "order-2 sign n=%d (%d,%d)", n, a, b);
        }
}

static std::vector<uint64_t> bitmap_of(const std::vector<cplx> &psi, int n) {
    std::vector<uint64_t> b(rdm::bitmap_words(n), 0);
    for (uint64_t i = 0; i < psi.size(); ++i)
        if (psi[i] != cplx(0.0, 0.0)) b[i >> 6] |= 1ull << (i & 63);
    return b;
}

static std::vector<uint64_t> shadow(const std::vector<uint64_t> &in, int n) {
    std::vector<uint64_t> out(in.size());
    for (uint64_t w = 0; w < in.size(); ++w) out[w] = rdm::shadow_word(in.data(), w, n);
    return out;
}

// the rows the way the device lists them: popcounts, exclusive prefix sums, set bits of each word from its start
static std::vector<uint64_t> row_list(const std::vector<uint64_t> &bm) {
    std::vector<uint64_t> start(bm.size() + 1, 0);
    for (size_t w = 0; w < bm.size(); ++w) start[w + 1] = start[w] + (uint64_t)__builtin_popcountll(bm[w]);
    std::vector<uint64_t> rows(start.back());
    for (size_t w = 0; w < bm.size(); ++w) {
        uint64_t m = bm[w], at = start[w];
        while (m) {
            rows[at++] = w * 64 + (uint64_t)__builtin_ctzll(m);
            m &= m - 1;
        }
    }
    return rows;
}

static void check_shadow_and_rows(const std::vector<cplx> &psi, int n, std::vector<uint64_t> rows_out[2]) {
    const uint64_t N = 1ull << n;
    std::vector<char> s0(N), s1(N, 0), s2(N, 0);
    for (uint64_t i = 0; i < N; ++i) s0[i] = psi[i] != cplx(0.0, 0.0);
    for (uint64_t K = 0; K < N; ++K)
        for (int b = 0; b < n; ++b)
            if (!(K >> b & 1) && s0[K | (1ull << b)]) s1[K] = 1;
    for (uint64_t K = 0; K < N; ++K)
        for (int b = 0; b < n; ++b)
            if (!(K >> b & 1) && s1[K | (1ull << b)]) s2[K] = 1;
    const std::vector<uint64_t> b0 = bitmap_of(psi, n), b1 = shadow(b0, n), b2 = shadow(b1, n);
    for (uint64_t K = 0; K < rdm::bitmap_words(n) * 64; ++K) {
        const bool in = K < N;
        CHECK(((b1[K >> 6] >> (K & 63)) & 1) == (uint64_t)(in ? s1[K] : 0), "shadow 1 n=%d K=%llu", n, (unsigned long long)K);
        CHECK(((b2[K >> 6] >> (K & 63)) & 1) == (uint64_t)(in ? s2[K] : 0), "shadow 2 n=%d K=%llu", n, (unsigned long long)K);
    }
    for (int o = 0; o < 2; ++o) {
        const std::vector<char> &s = o ? s2 : s1;
        const std::vector<uint64_t> rows = row_list(o ? b2 : b1);
        size_t want = 0;
        for (uint64_t K = 0; K < N; ++K) want += s[K];
        CHECK(rows.size() == want, "row count n=%d order=%d", n, o + 1);
        for (size_t i = 0; i < rows.size(); ++i) {
            CHECK(rows[i] < N && s[rows[i]], "row outside the shadow n=%d", n);
            if (i) CHECK(rows[i - 1] < rows[i], "rows not ascending n=%d", n);
        }
        rows_out[o] = rows;
    }
}

static void check_schedule(const rdm::Schedule &S) {
    CHECK(S.chunk_rows % S.tile_rows == 0 && S.slice_rows % S.tile_rows == 0 && S.chunk_rows >= S.tile_rows, "tile multiples");
    CHECK(S.workspace_bytes == (size_t)S.chunk_rows * S.row_bytes, "workspace bytes");
    CHECK((int64_t)S.slices * S.slice_rows >= S.chunk_rows && (int64_t)(S.slices - 1) * S.slice_rows < S.chunk_rows, "slices cover a chunk");
    CHECK(S.nchunks * S.chunk_rows >= S.rows && (S.nchunks == 0 || (S.nchunks - 1) * S.chunk_rows < S.rows), "chunks cover the rows");
    // every (row, block pair) once
    std::vector<int> seen((size_t)S.rows * S.npairs, 0);
    for (int64_t c = 0; c < S.nchunks; ++c) {
        const int64_t row0 = c * S.chunk_rows, cr = std::min(S.chunk_rows, S.rows - row0);
        for (int wg = 0; wg < S.npairs * S.slices; ++wg) {
            const int pair = wg / S.slices, slice = wg - pair * S.slices;
            const int64_t rb = (int64_t)slice * S.slice_rows, re = std::min(rb + S.slice_rows, cr);
            for (int64_t r0 = rb; r0 < re; r0 += S.tile_rows)
                for (int64_t r = r0; r < std::min<int64_t>(r0 + S.tile_rows, re); ++r) ++seen[(size_t)(row0 + r) * S.npairs + pair];
        }
    }
    for (int v : seen) CHECK(v == 1, "a (row, block pair) visited %d times", v);
    // block pairs: a bijection onto I <= J
    for (int p = 0; p < S.npairs; ++p) {
        int I, J;
        rdm::block_pair(p, S.nblk, &I, &J);
        CHECK(0 <= I && I <= J && J < S.nblk && rdm::block_pair_index(I, J, S.nblk) == p, "block pair %d", p);
    }
    for (int real = 0; real < 2; ++real) {
        std::vector<int> owner(rdm::GRAM_BLOCK, 0);
        for (int t = 0; t < 16; ++t)
            for (int j = 0; j < 4; ++j) ++owner[rdm::owned_column(real != 0, t, j)];
        for (int v : owner) CHECK(v == 1, "owned columns");
    }
}

// the slices of chunk c that hold no row (their workgroups return before they touch their slab)
static std::vector<int> empty_slices(const rdm::Schedule &S, int64_t c) {
    const int64_t cr = std::min(S.chunk_rows, S.rows - c * S.chunk_rows);
    std::vector<int> out;
    for (int s = 0; s < S.slices; ++s)
        if ((int64_t)s * S.slice_rows >= cr) out.push_back(s);
    return out;
}

// trips of k_rdm_rows' grid-stride loop over the largest chunk (grid: run_rdm), and of k_rdm_census' loop over the bitmap words
static int64_t rows_trips(const rdm::Schedule &S, int num_cus) {
    const uint64_t total = (uint64_t)std::min(S.chunk_rows, S.rows) * (uint64_t)S.wpad;
    const uint64_t grid = std::min<uint64_t>((total + 255) / 256, (uint64_t)num_cus * 16u);
    return grid ? (int64_t)((total + grid * 256 - 1) / (grid * 256)) : 0;
}
static int64_t census_trips(int n) {
    const uint64_t words = rdm::bitmap_words(n), grid = std::min<uint64_t>(1024, (words + 3) / 4);
    return (int64_t)((words + grid * 4 - 1) / (grid * 4));
}

// one case of tests/test_gpu_rdm_edges.py: what goes into plan() and what the test expects of the schedule
struct EdgeCase {
    const char *name;
    int n, order;
    bool real;
    int64_t rows, workspace_mb;
    int64_t chunks, last_chunk_rows;   // expected
    int nblk, slices;
    int64_t tiles_per_slice;
    int empty_in_last;                 // empty slices of the last launch
    bool rows_wrap, census_wraps;
};

static void check_edge_case(const EdgeCase &e) {
    const int cus = 256;
    const rdm::Schedule S = rdm::plan(e.n, e.order, e.real, e.rows, e.workspace_mb, cus);
    check_schedule(S);
    CHECK(S.elem_bytes == (e.real ? 8u : 16u), "%s: element size", e.name);
    CHECK(S.nchunks == e.chunks, "%s: %lld chunks", e.name, (long long)S.nchunks);
    CHECK(S.rows - (S.nchunks - 1) * S.chunk_rows == e.last_chunk_rows, "%s: last chunk of %lld rows", e.name,
          (long long)(S.rows - (S.nchunks - 1) * S.chunk_rows));
    CHECK(S.nblk == e.nblk && S.npairs == e.nblk * (e.nblk + 1) / 2, "%s: %d blocks", e.name, S.nblk);
    CHECK(S.slices == e.slices, "%s: %d slices", e.name, S.slices);
    CHECK(S.slice_rows == e.tiles_per_slice * S.tile_rows, "%s: %lld tiles per slice", e.name, (long long)(S.slice_rows / S.tile_rows));
    CHECK((S.nchunks > rdm::TIMED_CHUNKS_MAX) == (e.chunks > 64), "%s: timed", e.name);
    for (int64_t c = 0; c < S.nchunks; ++c) {
        const std::vector<int> empty = empty_slices(S, c);
        if (c + 1 < S.nchunks) {
            CHECK(empty.empty(), "%s: an empty slice in the full chunk %lld", e.name, (long long)c);
            continue;
        }
        CHECK((int)empty.size() == e.empty_in_last, "%s: %d empty slices in the last launch", e.name, (int)empty.size());
        for (size_t k = 0; k < empty.size(); ++k)   // exactly the slices behind the last row
            CHECK(empty[k] == S.slices - (int)empty.size() + (int)k, "%s: empty slice %d", e.name, empty[k]);
    }
    CHECK((rows_trips(S, cus) > 1) == e.rows_wrap, "%s: %lld trips of the rows kernel", e.name, (long long)rows_trips(S, cus));
    CHECK((census_trips(e.n) > 1) == e.census_wraps, "%s: %lld trips of the census", e.name, (long long)census_trips(e.n));
}

// what k_rdm_rows, k_rdm_gram and k_rdm_finish do, index for index (REAL: 8-byte elements, the imaginary parts are not carried)
static std::vector<cplx> replay(const std::vector<cplx> &psi, const std::vector<uint64_t> &rows, const rdm::Schedule &S) {
    std::vector<rdm::ColEntry> cols;
    rdm::build_columns(S.n, S.order, cols);
    const int ES = (int)S.elem_bytes, TR = S.tile_rows, UPR = rdm::GRAM_BLOCK * ES / 16;
    const int DPE = ES / 8;   // doubles per element
    std::vector<double> ws(S.workspace_bytes / 8), slabs(S.slab_elems * DPE, 0.0);
    std::vector<double> la(rdm::GRAM_TILE_BYTES / 8), lb(rdm::GRAM_TILE_BYTES / 8);
    for (int64_t c = 0; c < S.nchunks; ++c) {
        const int64_t row0 = c * S.chunk_rows, cr = std::min(S.chunk_rows, S.rows - row0);
        for (uint64_t e = 0; e < (uint64_t)cr * S.wpad; ++e) {   // k_rdm_rows
            const uint64_t r = e / S.wpad;
            const int64_t col = (int64_t)(e - r * S.wpad);
            cplx v = 0.0;
            if (col < S.width) {
                bool neg;
                const uint64_t src = rdm::column_source(rows[row0 + r], cols[col], &neg);
                if (src != ~0ull) v = neg ? -psi[src] : psi[src];
            }
            ws[e * DPE] = v.real();
            if (!S.real) ws[e * DPE + 1] = v.imag();
        }
        for (int wg = 0; wg < S.npairs * S.slices; ++wg) {   // k_rdm_gram
            const int pair = wg / S.slices, slice = wg - pair * S.slices;
            const int64_t rb = (int64_t)slice * S.slice_rows, re = std::min(rb + S.slice_rows, cr);
            if (rb >= re) continue;
            int I, J;
            rdm::block_pair(pair, S.nblk, &I, &J);
            std::vector<cplx> acc(256 * 16, 0.0);
            for (int64_t r0 = rb; r0 < re; r0 += TR) {
                for (int unit = 0; unit < rdm::GRAM_TILE_BYTES / 16; ++unit) {   // staging: 16-byte units
                    const int row = unit / UPR, cu = unit - row * UPR;
                    double a[2] = {0.0, 0.0}, b[2] = {0.0, 0.0};
                    if (r0 + row < re) {
                        const double *src = ws.data() + (size_t)(r0 + row) * S.row_bytes / 8;
                        std::memcpy(a, src + (size_t)I * rdm::GRAM_BLOCK * DPE + 2 * cu, 16);
                        std::memcpy(b, src + (size_t)J * rdm::GRAM_BLOCK * DPE + 2 * cu, 16);
                    }
                    std::memcpy(&la[2 * unit], a, 16);
                    std::memcpy(&lb[2 * unit], b, 16);
                }
                for (int tid = 0; tid < 256; ++tid) {
                    const int tx = tid & 15, ty = tid >> 4;
                    for (int k = 0; k < TR; ++k)
                        for (int i = 0; i < 4; ++i)
                            for (int j = 0; j < 4; ++j) {
                                cplx a, b;
                                if (S.real) {   // slot (i >> 1) * 16 + t holds columns owned_column(t, i & ~1) and the next
                                    a = la[2 * (k * UPR + (i >> 1) * 16 + ty) + (i & 1)];
                                    b = lb[2 * (k * UPR + (j >> 1) * 16 + tx) + (j & 1)];
                                } else {
                                    a = cplx(la[2 * (k * UPR + i * 16 + ty)], la[2 * (k * UPR + i * 16 + ty) + 1]);
                                    b = cplx(lb[2 * (k * UPR + j * 16 + tx)], lb[2 * (k * UPR + j * 16 + tx) + 1]);
                                }
                                acc[tid * 16 + i * 4 + j] += std::conj(a) * b;
                            }
                }
            }
            const size_t slab = (size_t)wg * rdm::GRAM_BLOCK * rdm::GRAM_BLOCK;
            for (int tid = 0; tid < 256; ++tid)
                for (int i = 0; i < 4; ++i)
                    for (int j = 0; j < 4; ++j) {
                        const size_t at = slab + (size_t)rdm::owned_column(S.real, tid >> 4, i) * rdm::GRAM_BLOCK + rdm::owned_column(S.real, tid & 15, j);
                        CHECK(at < S.slab_elems, "slab index");
                        slabs[at * DPE] += acc[tid * 16 + i * 4 + j].real();
                        if (!S.real) slabs[at * DPE + 1] += acc[tid * 16 + i * 4 + j].imag();
                    }
        }
    }
    const int64_t W = S.width;
    std::vector<cplx> out((size_t)W * W, cplx(NAN, NAN));
    for (int64_t p = 0; p < W; ++p)   // k_rdm_finish
        for (int64_t q = p; q < W; ++q) {
            const int I = (int)(p / rdm::GRAM_BLOCK), J = (int)(q / rdm::GRAM_BLOCK);
            const size_t first = (size_t)rdm::block_pair_index(I, J, S.nblk) * S.slices * rdm::GRAM_BLOCK * rdm::GRAM_BLOCK +
                                 (size_t)(p - (int64_t)I * rdm::GRAM_BLOCK) * rdm::GRAM_BLOCK + (size_t)(q - (int64_t)J * rdm::GRAM_BLOCK);
            double re = 0.0, im = 0.0;
            for (int s = 0; s < S.slices; ++s) {
                const size_t at = first + (size_t)s * rdm::GRAM_BLOCK * rdm::GRAM_BLOCK;
                re += slabs[at * DPE];
                if (!S.real) im += slabs[at * DPE + 1];
            }
            if (p == q) im = 0.0;
            out[p * W + q] = cplx(re, im);
            if (p != q) out[q * W + p] = cplx(re, -im);
        }
    return out;
}

// the definition, operator by operator: <a+_p a_q> resp. <a+_p a+_q a_s a_r> with the Jordan-Wigner sign of every single ladder step
static bool ladder(uint64_t &det, int n, int orb, bool create, int &sign) {
    const uint64_t bit = 1ull << (n - 1 - orb);
    if (((det & bit) != 0) == create) return false;
    if (occ_between(det, n, -1, orb) & 1) sign = -sign;
    det ^= bit;
    return true;
}
static std::vector<cplx> definition(const std::vector<cplx> &psi, int n, int order) {
    std::vector<std::vector<int>> cols;
    if (order == 1)
        for (int a = 0; a < n; ++a) cols.push_back({a});
    else
        for (int a = 0; a < n; ++a)
            for (int b = a + 1; b < n; ++b) cols.push_back({a, b});
    const size_t W = cols.size();
    std::vector<cplx> out(W * W, 0.0);
    for (uint64_t D = 0; D < psi.size(); ++D) {
        if (psi[D] == cplx(0.0, 0.0)) continue;
        for (size_t j = 0; j < W; ++j) {
            uint64_t K = D;
            int sj = 1;
            bool ok = true;
            for (int orb : cols[j]) ok = ok && ladder(K, n, orb, false, sj);   // a_r, then a_s
            if (!ok) continue;
            for (size_t i = 0; i < W; ++i) {
                uint64_t E = K;
                int si = sj;
                bool ok2 = true;
                for (auto it = cols[i].rbegin(); it != cols[i].rend(); ++it) ok2 = ok2 && ladder(E, n, *it, true, si);   // a+_q, then a+_p
                if (ok2) out[i * W + j] += std::conj(psi[E]) * psi[D] * (double)si;
            }
        }
    }
    return out;
}

int main(int argc, char **argv) {
    const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 7u;
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    for (int n = 1; n <= 9; ++n) {
        check_columns(n);
        for (int flavour = 0; flavour < 4; ++flavour) {   // dense complex, sparse complex, sparse real, a single determinant
            const uint64_t N = 1ull << n;
            std::vector<cplx> psi(N, 0.0);
            const double keep = flavour == 0 ? 1.0 : 0.15;
            for (uint64_t i = 0; i < N; ++i)
                if (u(rng) * 0.5 + 0.5 < keep) psi[i] = flavour == 2 ? cplx(u(rng), 0.0) : cplx(u(rng), u(rng));
            if (flavour == 3) {
                std::fill(psi.begin(), psi.end(), cplx(0.0, 0.0));
                psi[rng() % N] = 1.0;
            }
            std::vector<uint64_t> rows[2];
            check_shadow_and_rows(psi, n, rows);
            if (n > 7) continue;   // the replays below cost P^2 2^n
            bool real = true;
            for (const cplx &a : psi) real = real && a.imag() == 0.0;
            for (int order = 1; order <= 2; ++order) {
                if (order == 2 && n < 2) continue;
                const std::vector<cplx> want = definition(psi, n, order);
                // one chunk / the smallest workspace (one tile per chunk); few and many compute units (slice counts)
                for (int variant = 0; variant < 3; ++variant) {
                    const rdm::Schedule S = rdm::plan(n, order, real, (int64_t)rows[order - 1].size(), variant == 1 ? 0 : 1024, variant == 2 ? 1 : 256);
                    check_schedule(S);
                    if (variant == 1 && (int64_t)rows[order - 1].size() > S.tile_rows) CHECK(S.nchunks > 1, "the smallest workspace gives several chunks");
                    const std::vector<cplx> got = replay(psi, rows[order - 1], S);
                    double err = 0.0;
                    for (size_t i = 0; i < want.size(); ++i) err = std::max(err, std::abs(got[i] - want[i]));
                    CHECK(err <= 1e-13, "replay n=%d order=%d flavour=%d variant=%d: max error %.3e", n, order, flavour, variant, err);
                    const int64_t W = S.width;
                    for (int64_t p = 0; p < W; ++p)
                        for (int64_t q = 0; q < W; ++q)
                            CHECK(got[p * W + q] == std::conj(got[q * W + p]), "not Hermitian to the bit");
                }
            }
        }
    }
    // two column blocks (n = 12: P = 66, a last block of two valid columns, an off-diagonal block pair and its mirror) on sparse states
    for (int real = 0; real < 2; ++real) {
        const int n = 12;
        std::vector<cplx> psi(1ull << n, 0.0);
        for (int k = 0; k < 48; ++k) psi[rng() % psi.size()] = real ? cplx(u(rng), 0.0) : cplx(u(rng), u(rng));
        std::vector<uint64_t> rows[2];
        check_shadow_and_rows(psi, n, rows);
        const std::vector<cplx> want = definition(psi, n, 2);
        for (int mb : {1024, 0}) {
            const rdm::Schedule S = rdm::plan(n, 2, real != 0, (int64_t)rows[1].size(), mb, 8);
            check_schedule(S);
            CHECK(S.nblk == 2 && S.npairs == 3, "two column blocks");
            const std::vector<cplx> got = replay(psi, rows[1], S);
            double err = 0.0;
            for (size_t i = 0; i < want.size(); ++i) err = std::max(err, std::abs(got[i] - want[i]));
            CHECK(err <= 1e-13, "replay n=12 real=%d workspace=%d: max error %.3e", real, mb, err);
        }
    }
    // schedules of the sizes the device meets: many rows, several column blocks, a workspace that forces chunks
    for (int n : {12, 14, 17, 24})
        for (int order = 1; order <= 2; ++order)
            for (int real = 0; real < 2; ++real) {
                const rdm::Schedule S = rdm::plan(n, order, real != 0, 5000 + 13 * n, 1, 256);
                check_schedule(S);
            }
    // the cases of tests/test_gpu_rdm_edges.py (row counts: those of its seeded states), order 2 unless named otherwise
    const EdgeCase edge_cases[] = {
        // name            n  order real   rows    MB  chunks last blocks slices tiles/slice empty  rows wrap  census wraps
        {"A",             14, 2, false,  16369, 1024,   1, 16369, 2, 256,  4,  0, true,  false},
        {"A order 1",     14, 1, false,  16383, 1024,   1, 16383, 1, 256,  4,  0, false, false},
        {"B",             14, 2, true,   16369, 1024,   1, 16369, 2, 256,  2,  0, true,  false},
        {"C",             20, 2, true,  131981, 1024,   1, 131981, 3, 165, 25, 0, true,  true},
        {"C'",            20, 2, false, 131981, 1024,   1, 131981, 3, 169, 49, 0, true,  true},
        {"D",             12, 2, false,   4083,    0, 256,     3, 2,   1,  1,  0, false, false},
        {"D one chunk",   12, 2, false,   4083, 1024,   1,  4083, 2, 256,  1,  0, false, false},
        {"E",             13, 2, false,   1653,    1,   4,   117, 2,  32,  1, 24, false, false},
        {"F",             24, 2, true,  138006, 1024,   1, 138006, 5,  69, 63, 0, true,  true},
    };
    for (const EdgeCase &e : edge_cases) check_edge_case(e);
    for (int nblk = 1; nblk <= 7; ++nblk) {   // block_pair and block_pair_index are inverse, both ways
        int pair = 0;
        for (int I = 0; I < nblk; ++I)
            for (int J = I; J < nblk; ++J, ++pair) {
                int i, j;
                rdm::block_pair(pair, nblk, &i, &j);
                CHECK(i == I && j == J && rdm::block_pair_index(I, J, nblk) == pair, "block pair %d of %d blocks", pair, nblk);
            }
        CHECK(pair == nblk * (nblk + 1) / 2, "pairs of %d blocks", nblk);
    }
    if (g_fail) return 1;
    std::printf("rdm plan ok\n");
    return 0;
}
