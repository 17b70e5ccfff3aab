// Templates and inline helpers behind meshhost.h: the token readers and the
// parallel record parser of the mesh files, the parallel line formatter, and
// the mesh-file readers, Cuthill-McKee and SortElements over a solver's own
// node and element types.  Included by the solver sources only.
#pragma once

#include <algorithm>
#include <charconv>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <type_traits>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "fastnum.h"
#include "hostmem.h"
#include "hostpool.h"
#include "meshhost.h"

namespace xfemm {

namespace meshio {
// XFEMM_TRACE_LOAD=1: host milliseconds of the mesh-loading / renumbering stages on stderr
struct LoadTrace {
    bool on = std::getenv("XFEMM_TRACE_LOAD") != nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void mark(const char *what)
    {
        if (!on) return;
        const auto n = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[load] %-24s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count());
        t = n;
    }
};

// Token readers with fscanf's semantics: "%i" (strtol base 0: decimal, 0x..,
// leading-0 octal) and "%lf" (strtod).  Digit strings take a direct decimal
// path (the value strtol gives); everything else goes through strtol /
// strtod, so every value is the reference's fscanf value to the bit.  `nl`:
// the token must lie on the current line (line-parallel parsing).
inline bool ws(char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n' || c == '\v' || c == '\f'; }
inline bool skip_ws(const char *&p, bool nl)
{
    if (nl) {
        while (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\v' || *p == '\f') ++p;
        return *p && *p != '\n';
    }
    while (ws(*p)) ++p;
    return *p != 0;
}
inline bool read_int(const char *&p, int &v, bool nl)
{
    if (!skip_ws(p, nl)) return false;
    const char *q = p + (*p == '-' || *p == '+');
    if (*q >= '1' && *q <= '9') {   // plain decimal (no octal / hex prefix)
        long long a = 0;
        const char *r = q;
        while (*r >= '0' && *r <= '9' && r - q < 18) a = 10 * a + (*r++ - '0');
        if (!(*r >= '0' && *r <= '9') && a <= 2147483648LL) {
            v = (int)(*p == '-' ? -a : a);
            p = r;
            return true;
        }
    }
    char *end = nullptr;
    const long x = std::strtol(p, &end, 0);
    if (end == p) return false;
    v = (int)x;
    p = end;
    return true;
}
inline bool read_double(const char *&p, double &v, bool nl)
{
    if (!skip_ws(p, nl)) return false;
    const char *end = nullptr;   // (strtod's value and extent, exact fast path: fastnum.h)
    if (!fastnum::parse_double(p, v, &end)) return false;
    p = end;
    return true;
}

// [0, n) split over the host's cores (at most 16), f(begin, end) per part,
// on the persistent pool (hostpool.h)
template <class F>
void par_for(long long n, long long min_per_thread, F f)
{
    HostPool &pool = HostPool::get();
    const int T = (int)std::max<long long>(1, std::min<long long>((long long)pool.size(), n / std::max(1LL, min_per_thread)));
    if (T <= 1) {
        f(0LL, n);
        return;
    }
    pool.run(T, [&](int t) { f(n * t / T, n * (t + 1) / T); });
}

// v = n copies of val, the storage first-touched by the pool's threads
template <class T>
void par_assign(BigVec<T> &v, size_t n, const T &val)
{
    huge_reserve(v, n);
    v.clear();
    v.resize(n);   // (NoInitAlloc: nothing written)
    par_for((long long)n, 1 << 16, [&](long long a, long long b) {
        for (long long k = a; k < b; k++) ::new (&v[k]) T(val);
    });
}

// A whole mesh file in memory, read as the token stream fscanf sees.
struct TextBuf {
    // the file's bytes + a terminating NUL; not value-initialised (the
    // parallel reads below fill it, each thread faulting in its own pages),
    // on huge pages, kept for the next file of the mesh
    struct Bytes {
        HugeBuf<char> b;
        size_t n = 0;   // bytes incl. the NUL
        char *data() { return b.data(); }
        const char *data() const { return b.data(); }
        size_t size() const { return n; }
        char &operator[](size_t i) { return b[i]; }
    } d;
    size_t pos = 0;
    size_t hint = 0;      // bytes to allocate at least (the largest file to come)
    double ms_count = 0;  // (trace: the record-count pass of the last records())
    bool load(const std::string &path)
    {
        const int fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        if (::fstat(fd, &st) != 0) {
            ::close(fd);
            return false;
        }
        const size_t n = (size_t)std::max<off_t>(0, st.st_size);
        // (sized for the largest mesh file at the first load: .edge > .ele > .node for fmesher output)
        if (!d.b.allocate(std::max<size_t>(n + 1, hint))) {
            ::close(fd);
            return false;
        }
        // chunks of >= 4 MiB read side by side (pread: no shared file offset)
        const int T = (int)std::max<size_t>(1, std::min<size_t>(16, n >> 22));
        std::vector<size_t> got(T, 0);
        par_for(T, 1, [&](long long a, long long b) {
            for (long long t = a; t < b; ++t) {
                size_t o = n * t / T;
                const size_t e = n * (t + 1) / T;
                while (o < e) {
                    const ssize_t r = ::pread(fd, d.b.data() + o, e - o, (off_t)o);
                    if (r <= 0) break;
                    o += (size_t)r;
                    got[t] += (size_t)r;
                }
            }
        });
        ::close(fd);
        size_t tot = 0;
        for (size_t g : got) tot += g;
        if (tot != n) return false;
        d.b[n] = '\0';
        d.n = n + 1;
        pos = 0;
        return true;
    }
    bool next_int(int &v)
    {
        const char *p = d.data() + pos;
        if (!read_int(p, v, false)) return false;
        pos = (size_t)(p - d.data());
        return true;
    }
    // the first line's leading integer (fgets + sscanf "%i"), then the stream after that line
    bool header_int(int &v)
    {
        const char *nl = std::strchr(d.data(), '\n');
        std::string line(d.data(), nl ? (size_t)(nl - d.data()) : std::strlen(d.data()));
        pos = nl ? (size_t)(nl - d.data()) + 1 : d.size() - 1;
        return std::sscanf(line.c_str(), "%i", &v) == 1;
    }
    // `count` records from pos on, rec(p, index, nl) reading one record.
    // When every record sits on a line of its own (fmesher's layout) the lines
    // are parsed in parallel chunks -- the same values as the token stream;
    // any other layout (a record over several lines, extra tokens on a line)
    // is parsed as one sequential token stream, as fscanf reads it.
    template <class Rec>
    bool records(int count, Rec rec)
    {
        const char *base = d.data() + pos, *end = d.data() + d.size() - 1;
        const long long len = end - base;
        const int T = (int)std::max<long long>(1, std::min<long long>(HostPool::get().size(), len / (1 << 20)));
        bool ok = T > 1;
        const auto tc = std::chrono::steady_clock::now();
        ms_count = 0;
        if (ok) {
            // chunk starts at line starts; records (non-blank lines) per chunk
            std::vector<const char *> cs(T + 1);
            cs[0] = base;
            cs[T] = end;
            for (int t = 1; t < T; ++t) {
                const char *q = base + len * t / T;
                while (q < end && q[-1] != '\n') ++q;
                cs[t] = std::max(q, cs[t - 1]);
            }
            std::vector<long long> cnt(T + 1, 0);
            par_for(T, 1, [&](long long a, long long b) {
                for (long long t = a; t < b; ++t) {
                    // lines found by memchr; a line counts when a non-blank
                    // character precedes its end (leading blanks are few)
                    long long c = 0;
                    const char *q = cs[t], *const e = cs[t + 1];
                    while (q < e) {
                        const char *nl = static_cast<const char *>(std::memchr(q, '\n', (size_t)(e - q)));
                        const char *le = nl ? nl : e;
                        while (q < le && ws(*q)) ++q;
                        c += q < le;
                        q = nl ? nl + 1 : e;
                    }
                    cnt[t + 1] = c;
                }
            });
            for (int t = 0; t < T; ++t) cnt[t + 1] += cnt[t];
            ms_count = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tc).count();
            ok = cnt[T] >= count;
            std::vector<char> good(T, 1);
            if (ok)
                par_for(T, 1, [&](long long a, long long b) {
                    for (long long t = a; t < b; ++t) {
                        long long k = cnt[t];
                        const char *q = cs[t];
                        while (q < cs[t + 1] && k < count) {
                            const char *p = q;
                            if (!skip_ws(p, true)) {   // blank line
                                q = p + (*p == '\n');
                                continue;
                            }
                            if (!rec(p, (int)k, true) || skip_ws(p, true)) {   // short record or extra tokens
                                good[t] = 0;
                                return;
                            }
                            ++k;
                            q = p + (*p == '\n');
                        }
                    }
                });
            for (char g : good) ok = ok && g;
        }
        if (!ok) {   // the token stream, sequentially
            const char *p = base;
            for (int k = 0; k < count; ++k)
                if (!rec(p, k, false)) return false;
        }
        return true;
    }
};
inline double ms_since(std::chrono::steady_clock::time_point &t)
{
    const auto n = std::chrono::steady_clock::now();
    const double ms = std::chrono::duration<double, std::milli>(n - t).count();
    t = n;
    return ms;
}

// "%.17g" and "%i" as printf writes them (std::to_chars: the same correctly
// rounded digits and the same %g form), for the .ans's large sections
inline char *put_g17(char *p, double v) { return fastnum::put_g17(p, v); }   // (exact: fastnum.h)
inline char *put_i(char *p, int v) { return std::to_chars(p, p + 16, v).ptr; }
// lines [0, n): line(i, buf) writes line i (at most max_line chars) and returns
// its end; formatted in parallel chunks into huge-page buffers, then written
// in order by fwrite (one write of ~10 GB/s on the box; a shared mapping of
// the file was measured 5x slower, tools/lab/io_probe.cpp)
inline int format_chunks(int n) { return (int)std::max(1, std::min<int>(HostPool::get().size(), n / 8192)); }
template <class F>
MeshHost::Formatted format_lines(int n, int max_line, F line)
{
    const int T = format_chunks(n);
    MeshHost::Formatted f;
    f.buf.resize(T);
    f.len.assign(T, 0);
    par_for(T, 1, [&](long long t0, long long t1) {
        for (long long t = t0; t < t1; ++t) {
            const int a = (int)((long long)n * t / T), b = (int)((long long)n * (t + 1) / T);
            if (!f.buf[t].allocate((size_t)(b - a) * max_line + 1)) continue;   // (Formatted::ok() fails)
            char *q = f.buf[t].data();
            for (int i = a; i < b; ++i) q = line(i, q);
            f.len[t] = (size_t)(q - f.buf[t].data());
        }
    });
    return f;
}
inline bool write_formatted(FILE *fp, const MeshHost::Formatted &f)
{
    if (!f.ok()) return false;   // (a chunk's buffer could not be allocated)
    for (size_t t = 0; t < f.buf.size(); ++t)
        if (f.len[t]) fwrite(f.buf[t].data(), 1, f.len[t], fp);
    return true;
}
template <class F>
bool write_lines(FILE *fp, int n, int max_line, F line)
{
    return write_formatted(fp, format_lines(n, max_line, line));
}
}  // namespace meshio

template <class Node, class Decode>
bool MeshHost::read_node_file(meshio::TextBuf &tb, BigVec<Node> &meshnode, Decode decode)
{
    using namespace meshio;
    LoadTrace tr;
    if (!tb.load(PathName + ".node")) return false;
    tr.mark("  .node read");
    int k = 0;
    if (!tb.header_int(k)) return false;
    NumNodes = k;
    par_assign(meshnode, (size_t)std::max(0, k), Node());
    if (!tb.records(k, [&](const char *&p, int i, bool nl) {
            int a, m;
            double x, y;
            if (!read_int(p, a, nl) || !read_double(p, x, nl) || !read_double(p, y, nl) || !read_int(p, m, nl))
                return false;
            decode(meshnode[i], x, y, m);
            return true;
        }))
        return false;
    if (tr.on) std::fprintf(stderr, "[load]   (record count pass %.1f ms)\n", tb.ms_count);
    tr.mark("nodes");
    return true;
}

template <class Elem>
bool MeshHost::read_element_file(meshio::TextBuf &tb, BigVec<Elem> &meshele)
{
    using namespace meshio;
    LoadTrace tr;
    if (!tb.load(PathName + ".ele")) return false;
    tr.mark("  .ele read");
    int k = 0;
    if (!tb.header_int(k)) return false;
    NumEls = k;
    par_assign(meshele, (size_t)std::max(0, k), Elem());
    tr.mark("  element array");
    if (!tb.records(k, [&](const char *&p, int i, bool nl) {
            int a;
            Elem &elm = meshele[i];
            return read_int(p, a, nl) && read_int(p, elm.p[0], nl) && read_int(p, elm.p[1], nl) &&
                   read_int(p, elm.p[2], nl) && read_int(p, elm.lbl, nl);
        }))
        return false;
    if (tr.on) std::fprintf(stderr, "[load]   (record count pass %.1f ms)\n", tb.ms_count);
    tr.mark("  element records");
    return true;
}

template <class Elem, class BlockOf>
MeshHost::ElementCheck MeshHost::check_elements(BigVec<Elem> &meshele, int nl, int defaultLabel, BlockOf blockOf)
{
    using namespace meshio;
    // the first failing element (in file order) decides the error, as the
    // reference's sequential loop does (fsolver.cpp:593-626)
    const int k = NumEls;
    const int T = 64;
    std::vector<int> bad_at(T, -1), bad_code(T, 0);
    par_for(T, 1, [&](long long t0, long long t1) {
        for (long long t = t0; t < t1; ++t) {
            const int a = (int)((long long)k * t / T), b = (int)((long long)k * (t + 1) / T);
            for (int i = a; i < b; i++) {
                Elem &elm = meshele[i];
                elm.lbl--;
                if (elm.lbl < 0) elm.lbl = defaultLabel;
                int code = 0;
                if (elm.lbl < 0) code = 1;
                else if (elm.lbl >= nl) code = 2;
                else
                    for (int q = 0; q < 3; q++)
                        if (elm.p[q] < 0 || elm.p[q] >= NumNodes) code = 3;
                if (code) {
                    bad_at[t] = i;
                    bad_code[t] = code;
                    break;
                }
                elm.blk = blockOf(elm.lbl);
            }
        }
    });
    ElementCheck r;
    for (int t = 0; t < T; ++t)
        if (bad_at[t] >= 0) {
            r.index = bad_at[t];
            r.code = bad_code[t];
            break;
        }
    return r;
}

// meshele[k] = the old meshele[src(k)]: a second element array copy-constructed
// in parallel (no serial value-initialisation), then swapped in
template <class Elem, class Src>
bool MeshHost::permute_elements(BigVec<Elem> &meshele, Src src)
{
    using namespace meshio;
    BigVec<Elem> out;
    huge_reserve(out, (size_t)std::max(0, NumEls));
    out.resize((size_t)std::max(0, NumEls));   // (NoInitAlloc: written below, in parallel)
    par_for(NumEls, 1 << 16, [&](long long a, long long b) {
        // (the sources are scattered: each record is a cache miss, so the
        // one kPf ahead is requested while this one is copied)
        constexpr long long kPf = 16;
        for (long long k = a; k < b; k++) {
            if (k + kPf < b) __builtin_prefetch(&meshele[src(k + kPf)], 0, 0);
            ::new (&out[k]) Elem(meshele[src(k)]);
        }
    });
    meshele.swap(out);
    static_assert(std::is_trivially_destructible<Elem>::value, "uninitialised storage");
    return true;
}

template <class Elem>
int MeshHost::sort_mesh_elements(BigVec<Elem> &meshele)
{
    using namespace meshio;
    // comb sort on p0+p1+p2 (cuthill.cpp:39-86): the permutation from the
    // scores (sort_permutation), applied once
    LoadTrace tr;
    HugeBuf<unsigned> score;
    HugeBuf<int> perm;
    if (!score.allocate((size_t)std::max(1, NumEls)) || !perm.allocate((size_t)std::max(1, NumEls))) return false;
    par_for(NumEls, 1 << 16, [&](long long a, long long b) {
        for (long long k = a; k < b; k++) {
            const Elem &e = meshele[k];
            score[k] = (unsigned)((long long)e.p[0] + e.p[1] + e.p[2]);
        }
    });
    if (NumEls > 1 && !sort_permutation(score.data(), NumEls, perm.data())) return false;
    if (NumEls <= 1) return true;
    permute_elements(meshele, [&](long long k) { return perm[k]; });
    tr.mark("  permute");
    return true;
}

template <class Node, class Elem, class Hook>
int MeshHost::cuthill_mesh(BigVec<Node> &meshnode, BigVec<Elem> &meshele, bool deleteFiles, Hook renumbered)
{
    using namespace meshio;
    // reverse-less Cuthill-McKee of cuthill.cpp:88-390, on the .edge connectivity
    LoadTrace tr;
    const int n_lines = (int)edges_.size();
    BigVec<int> numcon, newnum, nxtnum;
    par_assign(numcon, (size_t)NumNodes, 0);
    par_assign(newnum, (size_t)NumNodes, -1);
    par_assign(nxtnum, (size_t)NumNodes, -1);
    // neighbour lists as CSR, each in the order the reference's lists get
    // their entries (edge order).  Thread t takes the edges of its range and
    // bins both ends by the node range that owns them (bucket (t, u)); owner u
    // then reads its buckets in t order -- every list in edge order, as the
    // sequential loop appends it -- counts, scans and fills its own nodes.
    // The edge array is read twice in all (not once per thread).
    BigVec<int> aptr, adj;
    par_assign(aptr, (size_t)NumNodes + 1, 0);
    huge_reserve(adj, 2 * edges_.size());
    adj.resize(2 * edges_.size());   // (every slot written by the fill below)
    {
        const int T = (int)std::max<long long>(1, std::min<long long>(HostPool::get().size(), (long long)n_lines / 65536));
        const int chunk = (int)std::max<long long>(1, ((long long)NumNodes + T - 1) / T);
        auto lo = [&](int u) { return (int)std::min<long long>(NumNodes, (long long)chunk * u); };
        auto elo = [&](int t) { return (long long)n_lines * t / T; };
        std::vector<long long> bc((size_t)T * T + 1, 0);   // bucket (t, u) at t * T + u: ends counted, then offsets
        par_for(T, 1, [&](long long t0, long long t1) {
            for (long long t = t0; t < t1; ++t) {
                long long *c = bc.data() + t * T;
                for (long long i = elo((int)t); i < elo((int)t + 1); ++i) {
                    c[edges_[i][0] / chunk]++;
                    c[edges_[i][1] / chunk]++;
                }
            }
        });
        // layout: owner u's region holds its buckets t = 0 .. T-1 in order
        std::vector<long long> off((size_t)T * T), ubase(T + 1, 0);
        long long o = 0;
        for (int u = 0; u < T; ++u) {
            ubase[u] = o;
            for (int t = 0; t < T; ++t) {
                off[(size_t)t * T + u] = o;
                o += bc[(size_t)t * T + u];
            }
        }
        ubase[T] = o;
        BigVec<std::array<int, 2>> ends;   // (owned end, other end)
        huge_reserve(ends, (size_t)o);
        ends.resize((size_t)o);
        par_for(T, 1, [&](long long t0, long long t1) {
            for (long long t = t0; t < t1; ++t) {
                long long *w = off.data() + t * T;
                for (long long i = elo((int)t); i < elo((int)t + 1); ++i) {
                    const int e0 = edges_[i][0], e1 = edges_[i][1];
                    ends[w[e0 / chunk]++] = {e0, e1};
                    ends[w[e1 / chunk]++] = {e1, e0};
                }
            }
        });
        par_for(T, 1, [&](long long u0, long long u1) {
            for (long long u = u0; u < u1; ++u) {
                for (long long k = ubase[u]; k < ubase[u + 1]; ++k) numcon[ends[k][0]]++;
                long long q = ubase[u];   // (= the ends owned by the ranges before u)
                for (int v = lo((int)u); v < lo((int)u + 1); ++v) {
                    aptr[v] = (int)q;
                    q += numcon[v];
                }
                std::vector<int> cur(aptr.begin() + lo((int)u), aptr.begin() + lo((int)u + 1));
                for (long long k = ubase[u]; k < ubase[u + 1]; ++k) adj[cur[ends[k][0] - lo((int)u)]++] = ends[k][1];
            }
        });
        aptr[NumNodes] = (int)ubase[T];
    }
    if (deleteFiles) remove_async({PathName + ".edge"});
    tr.mark("adjacency");
    // bubble sort by increasing connectivity: swaps only on a strict decrease,
    // so it is the stable sort of the list by numcon -- an insertion sort per
    // list gives the same order; lists are independent
    par_for(NumNodes, 1 << 14, [&](long long a, long long b) {
        for (long long n0 = a; n0 < b; n0++) {
            int *l = adj.data() + aptr[n0];
            const int m = aptr[n0 + 1] - aptr[n0];
            for (int q = 1; q < m; q++) {
                const int v = l[q], kv = numcon[v];
                int r = q;
                for (; r > 0 && numcon[l[r - 1]] > kv; --r) l[r] = l[r - 1];
                l[r] = v;
            }
        }
    });
    tr.mark("neighbour sort");
    long long j = numcon[0];
    int n0 = 0;
    for (long long i = 1; i < NumNodes; i++) {
        if (numcon[i] < j) {
            j = numcon[i];
            n0 = (int)i;
        }
        if (j == 2) i = n_lines;
    }
    newnum[n0] = 0;
    int n = 1;
    nxtnum[0] = n0;
    if (NumNodes > 1) {
        do {
            for (int t = aptr[n0]; t < aptr[n0 + 1]; ++t)
                if (const int c = adj[t]; newnum[c] < 0) {
                    newnum[c] = n;
                    nxtnum[n] = c;
                    n++;
                }
            const int nextpos = newnum[n0] + 1;
            if (nextpos >= NumNodes || nxtnum[nextpos] < 0) {
                if (n >= NumNodes) break;
                for (int i = 0; i < NumNodes; i++)
                    if (newnum[i] < 0) {
                        j = numcon[i];
                        n0 = i;
                        break;
                    }
                for (int i = 0; i < NumNodes; i++) {
                    if ((newnum[i] < 0) && (numcon[i] < j)) {
                        j = numcon[i];
                        n0 = i;
                    }
                    if (j == 2) break;
                }
                newnum[n0] = n;
                nxtnum[n] = n0;
                n++;
            } else {
                n0 = nxtnum[nextpos];
            }
        } while (n < NumNodes);
    }
    tr.mark("numbering");
    for (auto &p : pbclist) {
        p.x = newnum[p.x];
        p.y = newnum[p.y];
    }
    renumbered(newnum);
    int newwide = 0;
    {
        std::mutex mu;
        par_for(NumNodes, 1 << 16, [&](long long a0, long long a1) {
            int w = 0;
            for (long long a = a0; a < a1; a++)
                for (int t = aptr[a]; t < aptr[a + 1]; ++t) w = std::max(w, std::abs(newnum[a] - newnum[adj[t]]));
            std::lock_guard<std::mutex> g(mu);
            newwide = std::max(newwide, w);
        });
    }
    BandWidth = newwide + 1;
    par_for(NumEls, 1 << 16, [&](long long a, long long b) {
        for (long long k = a; k < b; k++)
            for (int q = 0; q < 3; q++) meshele[k].p[q] = newnum[meshele[k].p[q]];
    });
    // SortNodes (fsolver.cpp:1341-1353): node i moves to slot newnum[i]
    BigVec<Node> sorted;
    huge_reserve(sorted, (size_t)NumNodes);
    sorted.resize(NumNodes);   // (every slot written below: newnum is a permutation)
    par_for(NumNodes, 1 << 16, [&](long long a, long long b) {
        for (long long k = a; k < b; k++) ::new (&sorted[newnum[k]]) Node(meshnode[k]);
    });
    meshnode.swap(sorted);
    tr.mark("bandwidth + renumber");
    sort_mesh_elements(meshele);
    tr.mark("SortElements");
    return true;
}

}  // namespace xfemm
