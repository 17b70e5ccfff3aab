// Shared host side of the three file-based solvers (see meshhost.h): message
// hooks, mesh-file removal, the device bring-up thread, the comb sort of
// SortElements.
#include "meshhost.h"

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <immintrin.h>
#include <sys/stat.h>
#include <unistd.h>

#include "hostpool.h"
#include "meshhost_impl.h"

namespace xfemm {

int PrintWarningMsg(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    int r = vfprintf(stderr, fmt, ap);
    va_end(ap);
    return r;
}

using namespace meshio;

MeshHost::MeshHost() : WarnMessage(&PrintWarningMsg), PrintMessage(&PrintWarningMsg) {}

MeshHost::~MeshHost()
{
    join_hip_warmup();
    join_removals();
}

void MeshHost::start_hip_warmup()
{
    // XFEMM_NO_HIP_WARMUP=1 leaves the bring-up to the first device call
    if (hip_warm_.joinable() || std::getenv("XFEMM_NO_HIP_WARMUP")) return;
    const int dev = device;
    hip_warm_ = std::thread([dev] { (void)xfk_device_init(dev); });
}

void MeshHost::join_hip_warmup()
{
    if (hip_warm_.joinable()) hip_warm_.join();
}

// The mesh files the reference deletes once read (fsolver.cpp:711-716,
// cuthill.cpp:140): unlinking ~170 MB of page cache costs tens of ms, so it
// runs beside the rest of runSolver and is joined before runSolver returns.
void MeshHost::remove_async(std::vector<std::string> paths)
{
    removers_.emplace_back([paths = std::move(paths)] {
        for (const auto &p : paths) remove(p.c_str());
    });
}

void MeshHost::join_removals()
{
    for (auto &t : removers_) t.join();
    removers_.clear();
}

void MeshHost::warn(const std::string &msg)
{
    lastError = msg;
    WarnMessage("%s", msg.c_str());
}

// an existing output file is moved aside and unlinked beside the write
// (truncating ~130 MB of page cache in fopen costs ~7 ms); the new file is
// written whole.  A symlinked or hard-linked output keeps the reference's
// fopen("wt") behaviour (truncated in place: the link target, inode and
// permissions stay); the aside name is unique (mkstemp in the same directory,
// replaced by rename).
void MeshHost::clear_old_output(const std::string &path)
{
    struct stat st;
    if (::lstat(path.c_str(), &st) != 0 || !S_ISREG(st.st_mode) || st.st_nlink > 1 || st.st_size < (1 << 20))
        return;
    std::string aside = path + ".xfemm-old-XXXXXX";
    const int fd = ::mkstemp(&aside[0]);
    if (fd < 0) return;
    ::close(fd);
    if (::rename(path.c_str(), aside.c_str()) == 0) remove_async({aside});
    else ::unlink(aside.c_str());
}

bool MeshHost::read_edge_file(TextBuf &tb, std::vector<int> &marked_out)
{
    LoadTrace tr;
    if (!tb.load(PathName + ".edge")) return false;
    tr.mark("  .edge read");
    int nedge = 0, flag = 0;
    if (!tb.next_int(nedge) || !tb.next_int(flag)) return false;
    par_assign(edges_, (size_t)std::max(0, nedge), std::array<int, 3>{0, 0, 0});
    if (nedge > 0 && !tb.records(nedge, [&](const char *&p, int i, bool nl) {
            int a;
            auto &e = edges_[i];
            return read_int(p, a, nl) && read_int(p, e[0], nl) && read_int(p, e[1], nl) && read_int(p, e[2], nl);
        }))
        return false;
    if (tr.on) std::fprintf(stderr, "[load]   (record count pass %.1f ms)\n", tb.ms_count);
    tr.mark("edge records");
    const int T = 64;
    std::vector<char> bad(T, 0);
    std::vector<std::vector<int>> marked(T);
    par_for(T, 1, [&](long long t0, long long t1) {
        for (long long t = t0; t < t1; ++t) {
            const int a = (int)((long long)nedge * t / T), b = (int)((long long)nedge * (t + 1) / T);
            for (int i = a; i < b; i++) {
                const auto &e = edges_[i];
                if (e[0] < 0 || e[1] < 0 || e[0] >= NumNodes || e[1] >= NumNodes) {
                    bad[t] = 1;
                    break;
                }
                if (e[2] < 0) marked[t].push_back(i);
            }
        }
    });
    for (char c : bad)
        if (c) return false;
    marked_out.clear();
    for (auto &m : marked) marked_out.insert(marked_out.end(), m.begin(), m.end());
    return true;
}

namespace {
// one run of comb-sort compare-swaps x[i] <-> y[i] (score = high 32 bits,
// swap on a strict decrease); x and y do not overlap.  Branch-free: a wide
// pass meets random data, whose swaps mispredict half the time.  Returns
// nonzero when anything moved.
__attribute__((target("avx2"))) unsigned long long comb_swap_run_avx2(unsigned long long *__restrict x,
                                                                       unsigned long long *__restrict y, int n)
{
    __m256i anyv = _mm256_setzero_si256();
    int i = 0;
    for (; i + 4 <= n; i += 4) {
        const __m256i a = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(x + i));
        const __m256i b = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(y + i));
        // (scores < 2^32: the signed 64-bit compare of the shifted keys is the unsigned one)
        const __m256i m = _mm256_cmpgt_epi64(_mm256_srli_epi64(a, 32), _mm256_srli_epi64(b, 32));
        _mm256_storeu_si256(reinterpret_cast<__m256i *>(x + i), _mm256_blendv_epi8(a, b, m));
        _mm256_storeu_si256(reinterpret_cast<__m256i *>(y + i), _mm256_blendv_epi8(b, a, m));
        anyv = _mm256_or_si256(anyv, m);
    }
    unsigned long long any = (unsigned long long)_mm256_movemask_epi8(anyv);
    for (; i < n; ++i) {
        const unsigned long long a = x[i], b = y[i];
        const unsigned long long m = 0ULL - (unsigned long long)((a >> 32) > (b >> 32));
        x[i] = (a & ~m) | (b & m);
        y[i] = (b & ~m) | (a & m);
        any |= m;
    }
    return any;
}
unsigned long long comb_swap_run_plain(unsigned long long *__restrict x, unsigned long long *__restrict y, int n)
{
    unsigned long long any = 0;
    for (int i = 0; i < n; ++i) {
        const unsigned long long a = x[i], b = y[i];
        const unsigned long long m = 0ULL - (unsigned long long)((a >> 32) > (b >> 32));
        x[i] = (a & ~m) | (b & m);
        y[i] = (b & ~m) | (a & m);
        any |= m;
    }
    return any;
}
unsigned long long comb_swap_run(unsigned long long *x, unsigned long long *y, int n)
{
    static const bool avx2 = __builtin_cpu_supports("avx2");
    return avx2 ? comb_swap_run_avx2(x, y, n) : comb_swap_run_plain(x, y, n);
}

// Narrow comb passes as scans (see SortElements).  op(c, x): the carried
// entry c stays only on a strictly greater score; the all-zero key (score 0)
// is its identity from the left, so a class's first entry needs no special
// case.  Rows of g positions: lane c of a row is class c.
inline unsigned long long scan_op(unsigned long long c, unsigned long long x)
{
    const unsigned long long m = 0ULL - (unsigned long long)((c >> 32) > (x >> 32));
    return (c & m) | (x & ~m);
}
// red[c] = op(red[c], key[r g + c]) over `rows` rows
__attribute__((target("avx2"))) void scan_reduce_avx2(unsigned long long *red, const unsigned long long *key,
                                                       long long rows, int g)
{
    int c = 0;
    for (; c + 4 <= g; c += 4) {
        __m256i r = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(red + c));
        const unsigned long long *k = key + c;
        for (long long i = 0; i < rows; ++i, k += g) {
            const __m256i x = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(k));
            const __m256i m = _mm256_cmpgt_epi64(_mm256_srli_epi64(r, 32), _mm256_srli_epi64(x, 32));
            r = _mm256_blendv_epi8(x, r, m);
        }
        _mm256_storeu_si256(reinterpret_cast<__m256i *>(red + c), r);
    }
    for (; c < g; ++c) {
        unsigned long long r = red[c];
        const unsigned long long *k = key + c;
        for (long long i = 0; i < rows; ++i, k += g) r = scan_op(r, *k);
        red[c] = r;
    }
}
// car[c] = op(car[c], key[r g + c]) = c_k; out[r g + c] = the smaller-score of
// c_k and key[(r + 1) g + c] (c_k on ties) -- `rows` rows, each with its
// next row present; returns nonzero when some position took the next entry
__attribute__((target("avx2"))) unsigned long long scan_rows_avx2(unsigned long long *car,
                                                                   const unsigned long long *key,
                                                                   unsigned long long *out, long long rows, int g)
{
    unsigned long long any = 0;
    int c = 0;
    __m256i anyv = _mm256_setzero_si256();
    for (; c + 4 <= g; c += 4) {
        __m256i cv = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(car + c));
        const unsigned long long *k = key + c;
        unsigned long long *o = out + c;
        for (long long i = 0; i < rows; ++i, k += g, o += g) {
            const __m256i x = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(k));
            const __m256i nx = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(k + g));
            const __m256i m0 = _mm256_cmpgt_epi64(_mm256_srli_epi64(cv, 32), _mm256_srli_epi64(x, 32));
            cv = _mm256_blendv_epi8(x, cv, m0);
            const __m256i m = _mm256_cmpgt_epi64(_mm256_srli_epi64(cv, 32), _mm256_srli_epi64(nx, 32));
            _mm256_storeu_si256(reinterpret_cast<__m256i *>(o), _mm256_blendv_epi8(cv, nx, m));
            anyv = _mm256_or_si256(anyv, m);
        }
        _mm256_storeu_si256(reinterpret_cast<__m256i *>(car + c), cv);
    }
    any = (unsigned long long)_mm256_movemask_epi8(anyv);
    for (; c < g; ++c) {
        unsigned long long cc = car[c];
        const unsigned long long *k = key + c;
        unsigned long long *o = out + c;
        for (long long i = 0; i < rows; ++i, k += g, o += g) {
            cc = scan_op(cc, *k);
            const unsigned long long nx = k[g];
            const unsigned long long m = 0ULL - (unsigned long long)((cc >> 32) > (nx >> 32));
            *o = (nx & m) | (cc & ~m);
            any |= m;
        }
        car[c] = cc;
    }
    return any;
}
void scan_reduce_plain(unsigned long long *red, const unsigned long long *key, long long rows, int g)
{
    for (int c = 0; c < g; ++c) {
        unsigned long long r = red[c];
        const unsigned long long *k = key + c;
        for (long long i = 0; i < rows; ++i, k += g) r = scan_op(r, *k);
        red[c] = r;
    }
}
unsigned long long scan_rows_plain(unsigned long long *car, const unsigned long long *key, unsigned long long *out,
                                   long long rows, int g)
{
    unsigned long long any = 0;
    for (int c = 0; c < g; ++c) {
        unsigned long long cc = car[c];
        const unsigned long long *k = key + c;
        unsigned long long *o = out + c;
        for (long long i = 0; i < rows; ++i, k += g, o += g) {
            cc = scan_op(cc, *k);
            const unsigned long long nx = k[g];
            const unsigned long long m = 0ULL - (unsigned long long)((cc >> 32) > (nx >> 32));
            *o = (nx & m) | (cc & ~m);
            any |= m;
        }
        car[c] = cc;
    }
    return any;
}
void scan_reduce(unsigned long long *red, const unsigned long long *key, long long rows, int g)
{
    static const bool avx2 = __builtin_cpu_supports("avx2");
    if (avx2 && g >= 4) scan_reduce_avx2(red, key, rows, g);
    else scan_reduce_plain(red, key, rows, g);
}
unsigned long long scan_rows(unsigned long long *car, const unsigned long long *key, unsigned long long *out,
                             long long rows, int g)
{
    static const bool avx2 = __builtin_cpu_supports("avx2");
    return (avx2 && g >= 4) ? scan_rows_avx2(car, key, out, rows, g) : scan_rows_plain(car, key, out, rows, g);
}
}  // namespace

// The comb sort of SortElements (cuthill.cpp:39-86) on p0+p1+p2; not stable,
// restated exactly: the same comparisons and swaps, on packed (score,
// element) keys instead of the element records, which the caller permutes
// once at the end.  With a GPU (the solve needs one anyway) every pass runs on
// the device (xfk_sort_elements: ~2 ms instead of ~45 on 16 host cores);
// without one, or with XFEMM_HOST_SORT set, on the host below.
bool MeshHost::sort_permutation(const unsigned *score, int NumEls, int *perm)
{
    LoadTrace tr;
    join_hip_warmup();
    if (NumEls > 1 && !std::getenv("XFEMM_HOST_SORT") && xfk_device_count() > 0) {
        if (xfk_sort_elements(NumEls, score, device, perm) != XFK_OK) {
            warn(std::string("device element sort failed: ") + xfk_last_error() + "\n");
            return false;
        }
        tr.mark("  device comb sort");
        return true;
    }
    std::vector<unsigned long long> key, tmp;
    huge_reserve(key, (size_t)NumEls);
    huge_reserve(tmp, (size_t)NumEls);
    key.resize(NumEls);
    par_for(NumEls, 1 << 16, [&](long long a, long long b) {
        for (long long k = a; k < b; k++) {
            key[k] = ((unsigned long long)score[k] << 32) | (unsigned)k;
        }
    });
    // A pass with gap g compares (j, j + g) for j ascending: the steps of one
    // residue class j mod g touch only that class's entries, in ascending
    // order, so classes are independent.  Wide passes split the classes over
    // threads.  Narrow passes (few classes) use that a pass over one class is
    // a bubble pass: the element carried to position k is the prefix
    // "maximum" c_k = op(c_{k-1}, x_k), op(a, b) = score(a) > score(b) ? a : b
    // (a swap happens exactly when the carried score exceeds the next one:
    // ties keep their order), and position k receives
    // score(c_k) > score(x_{k+1}) ? x_{k+1} : c_k -- an associative scan, so
    // chunks of rows run in parallel from their classes' carries (computed
    // from per-chunk reductions): out of place, the same result as the
    // sequential pass
    HostPool &pool = HostPool::get();
    const int T = pool.size();
    auto scan_pass = [&](int g) -> bool {
        // chunks of whole rows (g positions each); every chunk but the last
        // holds every class, so the carries need no presence flags
        const long long n = NumEls;
        const long long R = (n + g - 1) / g;
        const int TT = (int)std::max<long long>(1, std::min<long long>(T, R / 64));
        std::vector<long long> q0(TT + 1);
        for (int t = 0; t <= TT; ++t) q0[t] = std::min(n, (R * t / TT) * g);
        std::vector<unsigned long long> red((size_t)TT * g), cin((size_t)TT * g);
        std::vector<char> sw(TT, 0);
        auto run = [&](auto fn) { pool.run(TT, fn); };
        run([&](int t) {   // per chunk and class: the op-reduction of its entries (from the identity 0)
            if (t == TT - 1) return;   // (the last chunk feeds no carry; the others are whole rows)
            unsigned long long *rd = red.data() + (size_t)t * g;
            std::fill(rd, rd + g, 0ULL);
            scan_reduce(rd, key.data() + q0[t], (q0[t + 1] - q0[t]) / g, g);
        });
        for (int t = 1; t < TT; ++t)   // carries into each chunk
            for (int c = 0; c < g; ++c) {
                const size_t i1 = (size_t)(t - 1) * g + c, i2 = (size_t)t * g + c;
                cin[i2] = t == 1 ? red[i1] : scan_op(cin[i1], red[i1]);
            }
        tmp.resize(NumEls);
        run([&](int t) {
            const long long a = q0[t], e = q0[t + 1];
            if (a >= e) return;
            std::vector<unsigned long long> car(g, 0ULL);   // chunk 0: the identity
            if (t > 0) std::copy(cin.begin() + (size_t)t * g, cin.begin() + (size_t)(t + 1) * g, car.begin());
            // whole rows whose next row is complete, then position by position
            const long long full = std::max(0LL, std::min((e - a) / g, (n - g - a) / g));
            unsigned long long any = scan_rows(car.data(), key.data() + a, tmp.data() + a, full, g);
            int c = 0;
            long long q = a + full * g;
            const long long lim = std::min(e, n - g);   // positions with a partner one gap on
            for (; q < lim; ++q) {
                const unsigned long long cc = scan_op(car[c], key[q]);   // c_k
                car[c] = cc;
                const unsigned long long nx = key[q + g];                 // x_{k+1}
                const unsigned long long m = 0ULL - (unsigned long long)((cc >> 32) > (nx >> 32));
                tmp[q] = (nx & m) | (cc & ~m);
                any |= m;
                if (++c == g) c = 0;
            }
            for (; q < e; ++q) {   // the last g positions: the carried entry lands
                tmp[q] = scan_op(car[c], key[q]);
                if (++c == g) c = 0;
            }
            sw[t] = any != 0;
        });
        key.swap(tmp);
        bool any = false;
        for (char c : sw) any |= c != 0;
        return any;
    };
    int gap = NumEls, i = 0;
    double ms_wide = 0, ms_narrow = 0;
    int n_wide = 0, n_narrow = 0;
    do {
        const auto tp = std::chrono::steady_clock::now();
        if (gap > 1) {
            gap = (gap * 10) / 13;
            if ((gap == 10) || (gap == 9)) gap = 11;
        }
        i = 0;
        if (T > 1 && gap >= 8 * T && NumEls >= (1 << 16)) {
            std::vector<char> sw(T, 0);
            const int g = gap;
            auto part = [&](int t) {
                const int r0 = (int)((long long)g * t / T), r1 = (int)((long long)g * (t + 1) / T);
                unsigned long long any = 0;
                for (long long b = 0; b + g < NumEls; b += g) {
                    // (the class range [r0, r1) of this block and its partners one gap on:
                    // disjoint, so the compare-swaps are independent -- branch-free)
                    const int re = (int)std::min<long long>(r1, NumEls - g - b);
                    any |= comb_swap_run(key.data() + b + r0, key.data() + b + r0 + g, re - r0);
                }
                sw[t] = any != 0;
            };
            pool.run(T, part);
            for (char c : sw) i |= c;
        } else if (T > 1 && NumEls >= (1 << 16)) {   // (narrow passes: few classes)
            i = scan_pass(gap) ? 1 : 0;
        } else {
            for (int j = 0; (j + gap) < NumEls; j++) {
                if ((key[j] >> 32) > (key[j + gap] >> 32)) {
                    std::swap(key[j], key[j + gap]);
                    i = 1;
                }
            }
        }
        const double dt = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp).count();
        if (T > 1 && gap >= 8 * T && NumEls >= (1 << 16)) ms_wide += dt, ++n_wide;
        else ms_narrow += dt, ++n_narrow;
    } while ((gap > 1) && (i > 0));
    if (tr.on)
        std::fprintf(stderr, "[load]   comb passes: %d wide %.1f ms, %d narrow %.1f ms\n", n_wide, ms_wide, n_narrow,
                     ms_narrow);
    tr.mark("  comb sort");
    par_for(NumEls, 1 << 16, [&](long long a, long long b) {
        for (long long k = a; k < b; k++) perm[k] = (int)(key[k] & 0xffffffffu);
    });
    return true;
}

}  // namespace xfemm
