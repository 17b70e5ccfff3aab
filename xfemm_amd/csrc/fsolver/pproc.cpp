// Reader of .res / .anh solution files and the host-side contour of the
// post-processors (see pproc.h).
#include "pproc.h"

#include <cmath>
#include <cstring>

#include "meshhost_impl.h"

namespace xfemm {

using namespace meshio;

void SolutionFile::clear()
{
    static_cast<PotProblemData &>(*this) = PotProblemData();
    geom = PotGeometry();
    NumNodes = NumEls = 0;
    for (auto *v : {&x, &y, &V}) BigVec<double>().swap(*v);
    for (auto *v : {&Q, &p, &lbl}) BigVec<int>().swap(*v);
    condV.clear();
    condq.clear();
}

namespace {

// The text after [Solution] as lines: chunks that start at line starts, the
// lines before each counted once (memchr), so that any range of lines is
// parsed by the chunks that hold it, side by side.
struct Lines {
    const char *base = nullptr, *end = nullptr;
    std::vector<const char *> cs;     // T + 1 chunk starts
    std::vector<long long> first;     // T + 1: lines before each chunk
    long long total() const { return first.back(); }

    void index(const char *b, const char *e)
    {
        base = b;
        end = e;
        const long long len = e - b;
        const int T = (int)std::max<long long>(1, std::min<long long>(HostPool::get().size(), len / (1 << 20)));
        cs.assign(T + 1, b);
        cs[T] = e;
        for (int t = 1; t < T; ++t) {
            const char *q = b + len * t / T;
            while (q < e && q[-1] != '\n') ++q;
            cs[t] = std::max(q, cs[t - 1]);
        }
        first.assign(T + 1, 0);
        par_for(T, 1, [&](long long a, long long z) {
            for (long long t = a; t < z; ++t) {
                long long c = 0;
                const char *q = cs[t], *const ce = cs[t + 1];
                while (q < ce) {
                    const char *nl = static_cast<const char *>(std::memchr(q, '\n', (size_t)(ce - q)));
                    ++c;   // (a last line without its newline counts)
                    q = nl ? nl + 1 : ce;
                }
                first[t + 1] = c;
            }
        });
        for (int t = 0; t < T; ++t) first[t + 1] += first[t];
    }

    // rec(p, k) for the lines l0 + k, k in [0, count), p at the line's start;
    // returns the lowest k whose rec failed, or -1
    template <class Rec>
    long long each(long long l0, long long count, Rec rec) const
    {
        const int T = (int)cs.size() - 1;
        std::vector<long long> bad(T, -1);
        par_for(T, 1, [&](long long a, long long z) {
            for (long long t = a; t < z; ++t) {
                long long l = first[t];
                if (first[t + 1] <= l0 || l >= l0 + count) continue;
                const char *q = cs[t], *const ce = cs[t + 1];
                while (q < ce && l < l0 + count) {
                    const char *nl = static_cast<const char *>(std::memchr(q, '\n', (size_t)(ce - q)));
                    if (l >= l0) {
                        const char *p = q;
                        if (!rec(p, l - l0)) {
                            bad[t] = l - l0;
                            break;
                        }
                    }
                    ++l;
                    q = nl ? nl + 1 : ce;
                }
            }
        });
        for (long long b : bad)
            if (b >= 0) return b;
        return -1;
    }
};

// nothing but blanks up to the end of the line
bool line_ends(const char *p)
{
    const char *q = p;
    return !skip_ws(q, true);
}

bool count_line(const Lines &L, long long l, int &n)
{
    n = -1;
    return L.each(l, 1, [&](const char *&p, long long) { return read_int(p, n, true) && line_ends(p) && n >= 0; }) < 0;
}

template <class T>
void big_resize(BigVec<T> &v, size_t n)
{
    huge_reserve(v, n);
    v.resize(n);   // (NoInitAlloc: every slot is written by the line parser)
}

}  // namespace

bool ReadSolutionFile(const std::string &path, PotentialKind kind, SolutionFile &out, std::string &err)
{
    out.clear();
    err.clear();
    auto fail = [&](const std::string &m) {
        out.clear();
        err = path + ": " + m;
        return false;
    };
    TextBuf tb;
    if (!tb.load(path)) return fail("couldn't read the file");
    const char *text = tb.d.data(), *const end = text + tb.d.size() - 1;
    // [Solution] on a line of its own
    const char *sol = nullptr, *after = nullptr;
    for (const char *q = text; q < end;) {
        const char *nl = static_cast<const char *>(std::memchr(q, '\n', (size_t)(end - q)));
        const char *le = nl ? nl : end;
        if (le - q >= 10 && q[0] == '[' && std::memcmp(q, "[Solution]", 10) == 0 && line_ends(q + 10)) {
            sol = q;
            after = nl ? nl + 1 : end;
            break;
        }
        if (!nl) break;
        q = nl + 1;
    }
    if (!sol) return fail(end == text ? "the file is empty: no [Solution]" : "no [Solution] section");
    {
        std::string perr;
        PotProblemData &hdr = out;
        if (!ParsePotentialText(text, (size_t)(sol - text), path, kind, hdr, &out.geom, perr)) return fail(perr);
    }
    const int npts = (int)out.geom.points.size();
    for (const auto &s : out.geom.segments)
        if (s.n0 < 0 || s.n1 < 0 || s.n0 >= npts || s.n1 >= npts) return fail("a segment names a point that is not there");
    for (const auto &a : out.geom.arcs)
        if (a.n0 < 0 || a.n1 < 0 || a.n0 >= npts || a.n1 >= npts) return fail("an arc segment names a point that is not there");

    Lines L;
    L.index(after, end);
    const long long total = L.total();
    long long at = 0;
    auto section = [&](const char *what, int &n) {
        if (at >= total) return fail(std::string("the file ends before the ") + what + " count (truncated)");
        if (!count_line(L, at, n)) return fail(std::string("the ") + what + " count is not a count");
        ++at;
        if (at + n > total)
            return fail(std::string("the ") + what + " count is " + std::to_string(n) + " but only " +
                        std::to_string(total - at) + " lines follow (truncated, or the count disagrees)");
        return true;
    };
    auto bad_line = [&](const char *what, long long k, int n) {
        return fail(std::string(what) + " line " + std::to_string(k) + " of " + std::to_string(n) +
                    " is not of its form (truncated, or the count disagrees with the lines present)");
    };

    int N = 0;
    if (!section("node", N)) return false;
    out.NumNodes = N;
    big_resize(out.x, (size_t)N);
    big_resize(out.y, (size_t)N);
    big_resize(out.V, (size_t)N);
    big_resize(out.Q, (size_t)N);
    long long b = L.each(at, N, [&](const char *&p, long long k) {
        return read_double(p, out.x[k], true) && read_double(p, out.y[k], true) && read_double(p, out.V[k], true) &&
               read_int(p, out.Q[k], true) && line_ends(p);
    });
    if (b >= 0) return bad_line("node", b, N);
    at += N;

    int NE = 0;
    if (!section("element", NE)) return false;
    out.NumEls = NE;
    big_resize(out.p, 3 * (size_t)NE);
    big_resize(out.lbl, (size_t)NE);
    b = L.each(at, NE, [&](const char *&p, long long k) {
        int *q = &out.p[3 * (size_t)k];
        return read_int(p, q[0], true) && read_int(p, q[1], true) && read_int(p, q[2], true) &&
               read_int(p, out.lbl[k], true) && line_ends(p);
    });
    if (b >= 0) return bad_line("element", b, NE);
    at += NE;
    {
        const int nl = (int)out.labellist.size();
        const int T = 64;
        std::vector<long long> badn(T, -1), badl(T, -1);
        par_for(T, 1, [&](long long t0, long long t1) {
            for (long long t = t0; t < t1; ++t) {
                const long long a = (long long)NE * t / T, z = (long long)NE * (t + 1) / T;
                for (long long i = a; i < z; ++i) {
                    for (int c = 0; c < 3; ++c)
                        if (badn[t] < 0 && (out.p[3 * i + c] < 0 || out.p[3 * i + c] >= N)) badn[t] = i;
                    if (badl[t] < 0 && (out.lbl[i] < 0 || out.lbl[i] >= nl)) badl[t] = i;
                }
            }
        });
        for (int t = 0; t < T; ++t) {
            if (badn[t] >= 0 && (badl[t] < 0 || badn[t] <= badl[t]))
                return fail("element " + std::to_string(badn[t]) + " has a node index outside the node range 0 .. " +
                            std::to_string(N - 1));
            if (badl[t] >= 0)
                return fail("element " + std::to_string(badl[t]) + " has label " + std::to_string(out.lbl[badl[t]]) +
                            ", beyond the label list of " + std::to_string(nl));
        }
    }

    int NC = 0;
    if (!section("conductor", NC)) return false;
    out.condV.assign((size_t)NC, 0.);
    out.condq.assign((size_t)NC, 0.);
    b = L.each(at, NC, [&](const char *&p, long long k) {
        return read_double(p, out.condV[k], true) && read_double(p, out.condq[k], true) && line_ends(p);
    });
    if (b >= 0) return bad_line("conductor", b, NC);
    at += NC;
    if (NC != (int)out.circproplist.size())
        return fail("the conductor count is " + std::to_string(NC) + ", the header defines " +
                    std::to_string(out.circproplist.size()));
    if (L.each(at, total - at, [](const char *&p, long long) { return line_ends(p); }) >= 0)
        return fail("text after the conductor lines");
    for (int i = 0; i < N; ++i)
        if (out.Q[i] < -2 || out.Q[i] >= NC)
            return fail("node " + std::to_string(i) + " has mark " + std::to_string(out.Q[i]) +
                        ", neither -2, -1 nor a conductor");
    return true;
}

// --- point location as the reference walks ---------------------------------------

void ElementWalk::build(const SolutionFile &f)
{
    const int NE = f.NumEls;
    cx.assign((size_t)NE, 0.);
    cy.assign((size_t)NE, 0.);
    rsqr.assign((size_t)NE, 0.);
    last = 0;
    par_for(NE, 1 << 16, [&](long long a, long long b) {
        for (long long i = a; i < b; ++i) {
            const int *n = &f.p[3 * (size_t)i];
            // PostProcessor::Ctr: the thirds summed in corner order
            double x = 0., y = 0.;
            for (int j = 0; j < 3; ++j) {
                x += f.x[n[j]] / 3.;
                y += f.y[n[j]] / 3.;
            }
            double r = 0.;
            for (int j = 0; j < 3; ++j) {
                const double dx = f.x[n[j]] - x, dy = f.y[n[j]] - y, q = dx * dx + dy * dy;
                if (q > r) r = q;
            }
            cx[i] = x;
            cy[i] = y;
            rsqr[i] = r;
        }
    });
}

bool ElementWalk::holds(const SolutionFile &f, double x, double y, int i) const
{
    if (i < 0 || i >= f.NumEls) return false;
    const int *p = &f.p[3 * (size_t)i];
    for (int j = 0; j < 3; j++) {
        const int k = j == 2 ? 0 : j + 1;
        const int pk = p[k], pj = p[j];
        // each edge is tested from its lower-numbered end, so that the two
        // elements sharing it decide with the same number
        if (pk > pj) {
            const double z = (f.x[pk] - f.x[pj]) * (y - f.y[pj]) - (f.y[pk] - f.y[pj]) * (x - f.x[pj]);
            if (z < 0) return false;
        } else {
            const double z = (f.x[pj] - f.x[pk]) * (y - f.y[pk]) - (f.y[pj] - f.y[pk]) * (x - f.x[pk]);
            if (z > 0) return false;
        }
    }
    return true;
}

int ElementWalk::find(const SolutionFile &f, double x, double y)
{
    const int sz = f.NumEls;
    if (sz <= 0 || (int)rsqr.size() != sz) return -1;
    int k = last;
    if (k < 0 || k >= sz) k = 0;
    last = k;
    if (holds(f, x, y, k)) return k;
    int hi = k, lo = k;
    for (int j = 0; j < sz; j += 2) {
        if (++hi >= sz) hi = 0;
        if (--lo < 0) lo = sz - 1;
        for (int e : {hi, lo}) {
            const double z = (cx[e] - x) * (cx[e] - x) + (cy[e] - y) * (cy[e] - y);
            if (z <= rsqr[e] && holds(f, x, y, e)) {
                last = e;
                return e;
            }
        }
    }
    return -1;
}

// --- the contour -------------------------------------------------------------

namespace {
struct Cx {
    double re, im;
};
inline Cx operator+(Cx a, Cx b) { return {a.re + b.re, a.im + b.im}; }
inline Cx operator-(Cx a, Cx b) { return {a.re - b.re, a.im - b.im}; }
inline Cx operator*(Cx a, Cx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
inline Cx operator*(double s, Cx a) { return {s * a.re, s * a.im}; }
inline Cx operator/(Cx a, double s) { return {a.re / s, a.im / s}; }
// abs(CComplex) (femmcomplex.cpp:749-757)
inline double cabs_(Cx z)
{
    if (z.re == 0 && z.im == 0) return 0.;
    if (std::fabs(z.re) > std::fabs(z.im)) return std::fabs(z.re) * std::sqrt(1. + (z.im / z.re) * (z.im / z.re));
    return std::fabs(z.im) * std::sqrt(1. + (z.re / z.im) * (z.re / z.im));
}
inline Cx cdiv(Cx a, Cx b)
{
    const double d = b.re * b.re + b.im * b.im;
    return {(a.re * b.re + a.im * b.im) / d, (a.im * b.re - a.re * b.im) / d};
}
inline double carg(Cx z) { return (z.re == 0 && z.im == 0) ? 0. : std::atan2(z.im, z.re); }

Cx point_of(const PotGeometry &g, int k) { return {g.points[k].x, g.points[k].y}; }

// FemmProblem::getCircle (FemmProblem.cpp:1523-1547)
void circle_of(const PotGeometry &g, const PotGeometry::Arc &arc, Cx &c, double &R)
{
    const Cx a0 = point_of(g, arc.n0), a1 = point_of(g, arc.n1);
    const double d = cabs_(a1 - a0);
    const Cx t = (a1 - a0) / d;
    const double tta = arc.ArcLength * kPi / 180.;
    R = d / (2. * std::sin(tta / 2.));
    c = a0 + Cx{d / 2., std::sqrt(R * R - d * d / 4.)} * t;
}

// shortestDistanceFromSegment (FemmProblem.cpp:2059-2076)
double dist_segment(const PotGeometry &g, double p, double q, const PotGeometry::Segment &s)
{
    const double x0 = g.points[s.n0].x, y0 = g.points[s.n0].y, x1 = g.points[s.n1].x, y1 = g.points[s.n1].y;
    double t = ((p - x0) * (x1 - x0) + (q - y0) * (y1 - y0)) / ((x1 - x0) * (x1 - x0) + (y1 - y0) * (y1 - y0));
    if (t > 1.) t = 1.;
    if (t < 0.) t = 0.;
    const double x2 = x0 + t * (x1 - x0), y2 = y0 + t * (y1 - y0);
    return std::sqrt((p - x2) * (p - x2) + (q - y2) * (q - y2));
}

// shortestDistanceFromArc (FemmProblem.cpp:2081-2101)
double dist_arc(const PotGeometry &g, Cx p, const PotGeometry::Arc &arc)
{
    double R;
    Cx c;
    circle_of(g, arc, c, R);
    const double d = cabs_(p - c);
    if (d == 0) return R;
    const Cx a0 = point_of(g, arc.n0), a1 = point_of(g, arc.n1);
    const Cx t = (p - c) / d;
    double l = cabs_(p - c - R * t);
    double z = carg(cdiv(t, a0 - c)) * 180 / kPi;
    if ((z > 0) && (z < arc.ArcLength)) return l;
    z = cabs_(p - a0);
    l = cabs_(p - a1);
    return z < l ? z : l;
}
}  // namespace

int ClosestGeometryPoint(const PotGeometry &g, double x, double y)
{
    if (g.points.empty()) return -1;
    auto dist = [&](int i) {
        return std::sqrt((x - g.points[i].x) * (x - g.points[i].x) + (y - g.points[i].y) * (y - g.points[i].y));
    };
    int idx = 0;
    double d0 = dist(0);
    for (int i = 0; i < (int)g.points.size(); i++) {
        const double d1 = dist(i);
        if (d1 < d0) {
            d0 = d1;
            idx = i;
        }
    }
    return idx;
}

int ClosestLabel(const PotProblemData &pr, double x, double y)
{
    if (pr.labellist.empty()) return -1;
    auto dist = [&](int i) {
        const CPBlockLabel &l = pr.labellist[i];
        return std::sqrt((x - l.x) * (x - l.x) + (y - l.y) * (y - l.y));
    };
    int idx = 0;
    double d0 = dist(0);
    for (int i = 0; i < (int)pr.labellist.size(); i++) {
        const double d1 = dist(i);
        if (d1 < d0) {
            d0 = d1;
            idx = i;
        }
    }
    return idx;
}

void ContourHost::add(double x, double y)
{
    if (pts.empty() || pts.back() != std::make_pair(x, y)) pts.emplace_back(x, y);
}

void ContourHost::add_from_node(const PotGeometry &g, double mx, double my)
{
    if (g.points.empty()) return;
    const int n0 = ClosestGeometryPoint(g, mx, my);
    int lineno = -1, arcno = -1;
    Cx z = point_of(g, n0);
    if (pts.empty()) {
        pts.emplace_back(z.re, z.im);
        return;
    }
    Cx y{pts.back().first, pts.back().second};
    if (y.re == z.re && y.im == z.im) return;
    const int n1 = ClosestGeometryPoint(g, y.re, y.im);
    Cx x = point_of(g, n1);
    // the last contour point is an input point: is (it, the new point) an
    // input segment or an arc segment?  The closest to (mx, my) wins.
    double d1 = 1.e08;
    bool reverseOrder = false;
    if (cabs_(x - y) < 1.e-08) {
        for (int k = 0; k < (int)g.segments.size(); k++) {
            const auto &s = g.segments[k];
            if ((s.n0 == n1 && s.n1 == n0) || (s.n0 == n0 && s.n1 == n1)) {
                const double d2 = std::fabs(dist_segment(g, mx, my, s));
                if (d2 < d1) {
                    lineno = k;
                    d1 = d2;
                }
            }
        }
        for (int k = 0; k < (int)g.arcs.size(); k++) {
            const auto &a = g.arcs[k];
            for (int rev = 1; rev >= 0; --rev)
                if (rev ? (a.n0 == n1 && a.n1 == n0) : (a.n0 == n0 && a.n1 == n1)) {
                    const double d2 = dist_arc(g, Cx{mx, my}, a);
                    if (d2 < d1) {
                        arcno = k;
                        lineno = -1;
                        reverseOrder = rev != 0;
                        d1 = d2;
                    }
                }
        }
    }
    auto behind = [&](Cx q) {   // q steps back onto the point before the last
        const size_t size = pts.size();
        return size > 1 && cabs_(Cx{pts[size - 2].first, pts[size - 2].second} - q) < 1.e-08;
    };
    if (lineno < 0 && arcno < 0) pts.emplace_back(z.re, z.im);
    if (lineno >= 0) {
        if (behind(z)) return;
        pts.emplace_back(z.re, z.im);
    }
    if (arcno >= 0) {
        const auto &a = g.arcs[arcno];
        double R;
        circle_of(g, a, x, R);
        const int arcsegments = (int)std::ceil(a.ArcLength / a.MaxSideLength);
        const double th = a.ArcLength * kPi / (180. * ((double)arcsegments));
        // (the contour starts at the arc's n0 when reverseOrder: counter-clockwise)
        const Cx rot = reverseOrder ? Cx{std::cos(th), std::sin(th)} : Cx{std::cos(th), -std::sin(th)};
        for (int i = 0; i < arcsegments; i++) {
            y = (y - x) * rot + x;
            // the last step lands on the input point itself, not beside it
            if (i == arcsegments - 1) y = z;
            if (behind(y)) return;
            pts.emplace_back(y.re, y.im);
        }
    }
}

void ContourHost::bend(double angle, double step)
{
    // bendContour (PostProcessor.cpp:772-820), as kernels.Contour.bend restates it
    if (angle == 0) return;
    if (step == 0) step = 1;
    const int k = (int)pts.size() - 1;
    if (k < 1) return;
    if (angle < -180. || angle > 180.) return;
    const int n = (int)std::ceil(std::fabs(angle / step));
    const double tta = angle * kPi / 180., dtta = tta / (double)n;
    const Cx a1{pts[k].first, pts[k].second}, a0{pts[k - 1].first, pts[k - 1].second};
    pts.pop_back();
    const Cx dz = a1 - a0;
    const double d = cabs_(dz);
    const double R = d / (2. * std::sin(std::fabs(tta / 2.)));
    const double ph = tta > 0 ? (kPi - tta) / 2. : (-1. * (kPi + tta)) / 2.;
    const Cx e{std::cos(ph), std::sin(ph)};
    const Cx s = (R / d) * dz;
    const Cx c = a0 + s * e;
    const Cx v = a0 - c;
    for (int q = 1; q <= n; q++) {
        const Cx r{std::cos((double)q * dtta), std::sin((double)q * dtta)};
        const Cx w = c + v * r;
        pts.emplace_back(w.re, w.im);
    }
}

}  // namespace xfemm
