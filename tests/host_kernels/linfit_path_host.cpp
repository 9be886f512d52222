// linfit_path_host -- the kernels `linfit::run` launches between its two stream synchronisations (kiwi_linfit.hpp), run on the
// HOST from their own source text under AddressSanitizer + UBSan (tests/test_host_kernels.py builds and runs this; it is never
// loaded into Python).  wave_exec.hpp runs a workgroup's lanes as threads; every device buffer is a heap allocation of exactly
// the element count the library's `ensure` calls ask for, so an index outside one is a sanitizer report.
//
//   linfit_path_host CASE OUT [--short BUFFER]
//
// CASE: what tests/host_kernel_cases.py wrote (database, receivers, references, tapers, sources, weights, K, and the oracle's
// plain synthetic strips, which stand in for what the accumulate kernel leaves in syn_d).  In launch order, with run_chunk's
// grids (kiwi_hip.hip run_chunk): geometry_kernel, cellgroup_kernel (cell mode), the audit of accumulate_grouped_kernel's
// addresses over the tables those two wrote, misfit_kernel with `proc`, global_kernel, linfit_gram_kernel<K>, linfit_solve_kernel<K>.
// kiwi_accum.inc itself (register-class assembly, LDS address-space casts, buffer loads) is not executed: the audit restates
// its walk over the centroid groups and every address formula of its build, apply and store, each cited by line.
// --short BUFFER: that ONE buffer of this program is allocated one element short -- the run must then end in a sanitizer report
// (the test of the detector).  BUFFER: recs, reft, tw, nbr have their last element read or written by a kernel at every set-up
// (tab and coef end in space no kernel touches, syn and proc in a slot's padding unless the last window is a multiple of four
// samples, the last pair flag is read in cell mode only); pairflag, syn, proc are accepted as well.
//
// Restated here, not moved, because the library's text is woven into its context object (kiwi_hip.hip): the row packing of
// kiwi_hip_set_gfdb (:1756-1822), the receiver geometry (:401-408, :1909-1951), the tapered branch of prepare() (:452-663), the
// buffer sizes and grids of run_chunk (:1078-1212, :1390-1453) and of linfit::run (kiwi_linfit.hpp run / launch_gram / launch).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "kiwi_common.hpp"
#include "kiwi_host.hpp"
#include "kiwi_geometry.hpp"
#include "kiwi_misfit.hpp"
using namespace kiwi;
#define KIWI_LINFIT_KERNELS_ONLY
#include "kiwi_linfit.hpp"

namespace {

// ------------------------------------------------------------------------------------------------ case and result files
// "KHK1", u32 count, then per array: char name[24], u32 type (0 int32, 1 float32, 2 float64, 3 uint8), u64 elements, the data
struct Arrays {
    struct A { unsigned type; std::vector<unsigned char> bytes; size_t n; };
    std::map<std::string, A> a;
    static size_t width(unsigned t) { return t == 2 ? 8 : (t == 3 ? 1 : 4); }
    void read(const char *path)
    {
        FILE *f = std::fopen(path, "rb");
        if (!f) throw std::runtime_error(std::string("cannot open ") + path);
        char magic[4];
        unsigned cnt = 0;
        if (std::fread(magic, 1, 4, f) != 4 || std::memcmp(magic, "KHK1", 4) != 0 || std::fread(&cnt, 4, 1, f) != 1) throw std::runtime_error("not a case file");
        for (unsigned i = 0; i < cnt; i++) {
            char name[25] = { 0 };
            unsigned type;
            unsigned long long n;
            if (std::fread(name, 1, 24, f) != 24 || std::fread(&type, 4, 1, f) != 1 || std::fread(&n, 8, 1, f) != 1) throw std::runtime_error("truncated case file");
            A x{ type, std::vector<unsigned char>((size_t)n * width(type)), (size_t)n };
            if (!x.bytes.empty() && std::fread(x.bytes.data(), 1, x.bytes.size(), f) != x.bytes.size()) throw std::runtime_error("truncated case file");
            a[name] = std::move(x);
        }
        std::fclose(f);
    }
    void write(const char *path) const
    {
        FILE *f = std::fopen(path, "wb");
        if (!f) throw std::runtime_error(std::string("cannot write ") + path);
        const unsigned cnt = (unsigned)a.size();
        std::fwrite("KHK1", 1, 4, f);
        std::fwrite(&cnt, 4, 1, f);
        for (auto &kv : a) {
            char name[24] = { 0 };
            std::snprintf(name, sizeof(name), "%s", kv.first.c_str());
            const unsigned long long n = kv.second.n;
            std::fwrite(name, 1, 24, f); std::fwrite(&kv.second.type, 4, 1, f); std::fwrite(&n, 8, 1, f);
            if (!kv.second.bytes.empty()) std::fwrite(kv.second.bytes.data(), 1, kv.second.bytes.size(), f);
        }
        std::fclose(f);
    }
    bool has(const std::string &k) const { return a.count(k) != 0; }
    template <class T> std::vector<T> get(const std::string &k, unsigned type) const
    {
        auto it = a.find(k);
        if (it == a.end()) throw std::runtime_error("case file has no '" + k + "'");
        if (it->second.type != type) throw std::runtime_error("'" + k + "' has another type");
        std::vector<T> v(it->second.n);
        if (!v.empty()) std::memcpy(v.data(), it->second.bytes.data(), it->second.bytes.size());
        return v;
    }
    std::vector<int> i32(const std::string &k) const { return get<int>(k, 0); }
    std::vector<float> f32(const std::string &k) const { return get<float>(k, 1); }
    std::vector<double> f64(const std::string &k) const { return get<double>(k, 2); }
    std::vector<unsigned char> u8(const std::string &k) const { return get<unsigned char>(k, 3); }
    template <class T> void put(const std::string &k, unsigned type, const T *p, size_t n)
    {
        A x{ type, std::vector<unsigned char>(n * sizeof(T)), n };
        if (n) std::memcpy(x.bytes.data(), p, n * sizeof(T));
        a[k] = std::move(x);
    }
    void put(const std::string &k, const std::vector<int> &v) { put(k, 0, v.data(), v.size()); }
    void put(const std::string &k, const std::vector<float> &v) { put(k, 1, v.data(), v.size()); }
    void put(const std::string &k, const std::vector<double> &v) { put(k, 2, v.data(), v.size()); }
};

// ------------------------------------------------------------------------------------------------ "device" buffers
std::string g_short;                         // --short: the buffer that gets one element less than it should

template <class T> struct Buf {
    T *p = nullptr;
    size_t n = 0, have = 0;                  // the count the library asks for (what the audit bounds against); the count allocated
    void alloc(const char *name, size_t count)
    {
        std::free(p);
        n = count;
        have = (g_short == name && count > 0) ? count - 1 : count;
        p = (T *)std::malloc(have * sizeof(T));              // exactly: the sanitizer's red zone starts at the next byte
        if (!p && have) throw std::bad_alloc();
    }
    void fill_bytes(int v) { if (have) std::memset(p, v, have * sizeof(T)); }
    ~Buf() { std::free(p); }
};

constexpr int kTabSentinel = 0x7f7f7f7f;     // (KIWI_HIP_POISON's byte, kiwi_hip.hip:1091-1095)
constexpr unsigned kCoefSentinel = 0x7f7f7f7fu;

[[noreturn]] void finding(const std::string &what)
{
    std::fprintf(stderr, "AUDIT: %s\n", what.c_str());
    std::fflush(stderr);
    std::exit(4);
}
#define AUDIT(cond, ...)                                                                            \
    do { if (!(cond)) { char b_[512]; std::snprintf(b_, sizeof(b_), __VA_ARGS__); finding(std::string(#cond) + ": " + b_); } } while (0)

struct HostReceiver {                        // kiwi_hip.hip:77-87
    GeoCoords origin;
    float depth = 0.f;
    bool enabled = true;
    int ncomp = 0;
    int comp[kMaxComp] = { 0 };
    struct Ref { int first = 0; std::vector<float> data; } ref[kMaxComp];
    Plf taper;
    double azi0 = 0, bazi0 = 0, dist0 = 0;
};

int component_id(char ch)                    // kiwi_hip.hip:394-399 (receiver.f90:294-307)
{
    static const char names[] = "wsulc?ardne";
    for (int i = 0; i < 11; i++) if (names[i] == ch) return i - 5;
    return 0;
}

int fold_halfwidth(float risetime, float dt) // kiwi_hip.hip:410-415
{
    if (!(risetime > 0.f)) return 0;
    const int n = 1 + 2 * (int)std::round(0.5f * risetime / dt);
    return (n - 1) / 2;
}

template <class F> void by_basis(int K, F &&f)       // kiwi_group_run.hpp:8-20
{
    switch (K) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    case 7: f(std::integral_constant<int, 7>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
    }
}

struct AuditCount { long long tiles = 0, groups = 0, loads = 0, stores = 0, applies = 0, skipped_records = 0; };

int run(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: linfit_path_host CASE OUT [--short BUFFER]\n"); return 2; }
    for (int i = 3; i + 1 < argc; i++) if (std::strcmp(argv[i], "--short") == 0) g_short = argv[i + 1];
    Arrays in, out;
    in.read(argv[1]);
    auto &ex = hostexec::exec();

    // ---- database: kiwi_hip_set_gfdb, kiwi_hip.hip:1756-1822
    const std::vector<int> dims = in.i32("gf_dims");
    const std::vector<float> gmeta = in.f32("gf_meta");
    const int nx = dims[0], nz = dims[1], ng = dims[2], L = dims[3];
    const std::vector<float> gdata = in.f32("gf_data");
    const std::vector<int> gfirst = in.i32("gf_first"), gnsamp = in.i32("gf_nsamp");
    const size_t nrows = (size_t)nx * nz * ng;
    if (ng != 8 && ng != 10) throw std::runtime_error("ng must be 8 or 10");
    if (gdata.size() != nrows * (size_t)L || gfirst.size() != nrows || gnsamp.size() != nrows) throw std::runtime_error("database arrays do not fit their dimensions");
    int lmax = 1;
    for (size_t i = 0; i < nrows; i++) {
        if (gnsamp[i] < 0 || gnsamp[i] > L) throw std::runtime_error("nsamp out of range");
        lmax = std::max(lmax, gnsamp[i]);
    }
    const int pitch = (kRowPad + lmax + kHalo + 32 + 3) / 4 * 4;                       // :1772
    Buf<float> G;
    Buf<int2> span;
    Buf<unsigned char> endz;
    G.alloc("G", nrows * (size_t)pitch); span.alloc("span", nrows); endz.alloc("endz", nrows);
    bool gaps = false;
    for (size_t row = 0; row < nrows; row++) {                                         // :1791-1803
        float *d = G.p + row * (size_t)pitch;
        const int n = gnsamp[row];
        const float *src = gdata.data() + row * (size_t)L;
        for (int k = 0; k < kRowPad; k++) d[k] = 0.f;
        for (int k = 0; k < n; k++) d[kRowPad + k] = src[k];
        const float tail = n > 0 ? src[n - 1] : 0.f;
        for (int k = kRowPad + n; k < pitch; k++) d[k] = tail;
        span.p[row] = make_int2(gfirst[row], gfirst[row] + n - 1);
        if (n <= 0) gaps = true;
        endz.p[row] = (tail == 0.f) ? 1 : 0;
    }
    const GfMeta gm{ nx, nz, ng, pitch, gmeta[0], gmeta[1], gmeta[2], gmeta[3], gmeta[4] };
    bool db_simple = !gaps;                                                            // :1811-1817
    for (size_t node = 0; db_simple && node < (size_t)nx * nz; node++)
        for (int ig = 0; ig < ng; ig++)
            if (span.p[node * ng + ig].x != span.p[node * ng].x || !endz.p[node * ng + ig]) { db_simple = false; break; }
    const float dt = gm.dt;

    // ---- receivers and the source location: :1909-1951, :401-408
    const std::vector<int> interp = in.i32("interp");
    const int bilinear = interp[0] ? 1 : 0, xus = interp[1], zus = interp[2];
    const std::vector<float> origin = in.f32("origin");
    GeoCoords src_origin;
    src_origin.lat = (double)d2r(origin[0]);
    src_origin.lon = (double)d2r(origin[1]);
    const std::vector<double> rlat = in.f64("rec_lat"), rlon = in.f64("rec_lon");
    const std::vector<float> rdepth = in.f32("rec_depth");
    const std::vector<unsigned char> rcomps = in.u8("rec_comps");
    const std::vector<int> renabled = in.i32("rec_enabled");
    const int nrec = (int)rlat.size();
    std::vector<HostReceiver> recv((size_t)nrec);
    const std::vector<int> ref_ofs = in.i32("ref_ofs"), ref_first = in.i32("ref_first"), taper_ofs = in.i32("taper_ofs");
    const std::vector<float> ref_data = in.f32("ref_data"), taper_x = in.f32("taper_x"), taper_y = in.f32("taper_y");
    {
        int slot = 0;
        for (int i = 0; i < nrec; i++) {
            HostReceiver &r = recv[i];
            r.origin.lat = d2r(rlat[i]); r.origin.lon = d2r(rlon[i]);
            r.depth = rdepth[i];
            const char *cs = (const char *)rcomps.data() + (size_t)i * 8;
            const int nc = (int)strnlen(cs, 8);
            if (nc > kMaxComp) throw std::runtime_error("too many components");
            for (int k = 0; k < nc; k++) { r.comp[k] = component_id(cs[k]); if (!r.comp[k]) throw std::runtime_error("unknown component"); }
            r.ncomp = nc;
            r.enabled = nc > 0 && renabled[i] != 0;
            for (int k = 0; k < nc; k++, slot++) {
                r.ref[k].first = ref_first[slot];
                r.ref[k].data.assign(ref_data.begin() + ref_ofs[slot], ref_data.begin() + ref_ofs[slot + 1]);
            }
            r.taper.x.assign(taper_x.begin() + taper_ofs[i], taper_x.begin() + taper_ofs[i + 1]);
            r.taper.y.assign(taper_y.begin() + taper_ofs[i], taper_y.begin() + taper_ofs[i + 1]);
            azibazi(src_origin, r.origin, r.azi0, r.bazi0);
            r.dist0 = distance_accurate50m(src_origin, r.origin);
        }
    }

    // ---- sources: the uploaded centroid tables (kiwi_hip.hip set_centroids, :2160-2301)
    std::vector<float> cent, moment, risetime;
    std::vector<int> cent_ofs;
    const int sourcetype = in.i32("sourcetype")[0];
    if (sourcetype == 6) {                   // `moment_tensor`: the library's own discretiser (kiwi_host.hpp)
        const std::vector<float> params = in.f32("params");
        const float edt = in.f32("effective_dt")[0];
        const int np = source_nparams(6), ns = (int)params.size() / np;
        cent_ofs.push_back(0);
        for (int s = 0; s < ns; s++) {
            DiscreteSource ds;
            if (!discretize(6, params.data() + (size_t)s * np, edt, ds)) throw std::runtime_error("a source did not discretise");
            for (auto &c : ds.centroids) { const float row[10] = { c.north, c.east, c.depth, c.time, c.m[0], c.m[1], c.m[2], c.m[3], c.m[4], c.m[5] }; cent.insert(cent.end(), row, row + 10); }
            cent_ofs.push_back((int)cent.size() / 10);
            moment.push_back(ds.moment); risetime.push_back(ds.risetime);
        }
    } else {                                 // tables made by the caller (the eikonal types: ko.discretize_eikonal, bit for bit the library's)
        cent = in.f32("cent"); cent_ofs = in.i32("cent_ofs"); moment = in.f32("moment"); risetime = in.f32("risetime");
    }
    const int nsrc = (int)moment.size();
    if ((int)cent_ofs.size() != nsrc + 1 || (size_t)cent_ofs[nsrc] * 10 != cent.size() || (int)risetime.size() != nsrc) throw std::runtime_error("centroid tables do not fit");
    float max_risetime = 0.f;
    for (int s = 0; s < nsrc; s++) max_risetime = std::max(max_risetime, risetime[s]);            // :2176-2177
    double points_per_centroid = 0.0;                                                              // :2263-2275
    {
        long long npts = 0, ncen = 0;
        const int stride = std::max(1, nsrc / 64);
        for (int s = 0; s < nsrc; s += stride) {
            const float *ce = cent.data() + (size_t)cent_ofs[s] * 10;
            const int nc = cent_ofs[s + 1] - cent_ofs[s];
            for (int k = 0; k < nc; k++) {
                const float *p = ce + (size_t)k * 10, *q = p - 10;
                if (k == 0 || !(p[0] == q[0] && p[1] == q[1] && p[2] == q[2])) npts++;
            }
            ncen += nc;
        }
        points_per_centroid = ncen > 0 ? (double)npts / (double)ncen : 0.0;
    }
    const std::vector<int> fitp = in.i32("fit");
    const int K = fitp[0], anarchy = fitp[1] ? 1 : 0;
    if (K < 1 || K > linfit::kMaxBasis || nsrc % K != 0) throw std::runtime_error("K does not fit");
    const int ngroup = nsrc / K;
    const float syn_factor = in.f32("syn_factor")[0];

    // ---- prepare(), tapered branch: kiwi_hip.hip:452-663
    const int hs = fold_halfwidth(max_risetime, dt);                                              // :469-470
    const int halo = hs > 0 ? hs + 2 : 0;
    std::vector<RecvDev> rd((size_t)nrec);
    std::vector<CompDev> comps;
    std::vector<float> reft, tw, norm_h;
    std::vector<int> recfirst;
    size_t synofs = 0;
    int max_wlen = 0;
    std::vector<int> rec_win;
    for (int ir = 0; ir < nrec; ir++) {                                                            // :506-624
        HostReceiver &r = recv[ir];
        RecvDev &d = rd[ir];
        std::memset(&d, 0, sizeof(d));
        d.azi0 = r.azi0; d.bazi0 = r.bazi0; d.dist0 = r.dist0;
        d.depth = r.depth;
        d.cl0 = (float)std::cos(r.bazi0 + (double)kPi);
        d.sl0 = (float)std::sin(r.bazi0 + (double)kPi);
        d.enabled = r.enabled && r.ncomp > 0;
        d.ncomp = r.ncomp;
        d.sd = 0.f;
        for (int k = 0; k < r.ncomp; k++) {
            d.comp[k] = std::abs(r.comp[k]);
            d.sign[k] = r.comp[k] < 0 ? -1.f : 1.f;
            if (d.comp[k] == 3) { d.has_d = 1; d.sd = d.sign[k]; } else d.need_h = 1;
        }
        rec_win.push_back(0); rec_win.push_back(0); rec_win.push_back(0); rec_win.push_back(0);
        if (!d.enabled) continue;
        if (!r.taper.defined()) throw std::runtime_error("an enabled receiver has no taper: linear_fit refuses it (kiwi_linfit.hpp check_setup)");
        for (int k = 0; k < r.ncomp; k++) if (r.ref[k].data.empty()) throw std::runtime_error("an enabled receiver component has no reference");
        int w[2];
        discrete_plf_span(r.taper, dt, w);
        if (w[1] < w[0]) throw std::runtime_error("empty taper span");
        const int wlen = w[1] - w[0] + 1;
        d.wbeg = w[0] - halo;
        d.wlen = wlen + 2 * halo;
        max_wlen = std::max(max_wlen, d.wlen);
        rec_win[4 * ir] = w[0]; rec_win[4 * ir + 1] = w[1]; rec_win[4 * ir + 2] = d.wbeg; rec_win[4 * ir + 3] = d.wlen;
        std::vector<float> tww((size_t)wlen, 1.f);
        plf_taper_array(r.taper, tww.data(), w[0], w[1], dt, IP_COS);
        recfirst.push_back((int)comps.size());
        d.slot0 = (int)comps.size();
        for (int k = 0; k < r.ncomp; k++) {
            const auto &rf = r.ref[k];
            CompDev cd;
            std::memset(&cd, 0, sizeof(cd));
            cd.synofs = (int)synofs; cd.halo = halo; cd.w0 = w[0]; cd.wlen = wlen;
            cd.refofs = (int)reft.size(); cd.rec = ir;
            cd.fl_lo = 0; cd.fl_ns = 1; cd.refxofs = 0;
            cd.untapered = 0;
            cd.vertical = std::abs(r.comp[k]) == 3 ? 1 : 0;
            { const int a = std::abs(r.comp[k]); cd.spankind = a == 3 ? 3 : (a == 1 ? 0 : (a == 2 ? 1 : 2)); }
            d.synofs[k] = (int)synofs;
            d.refofs[k] = cd.refofs;
            synofs += ((size_t)d.wlen + 3) / 4 * 4;
            const int f0 = rf.first, f1 = rf.first + (int)rf.data.size() - 1;
            cd.rf0 = f0; cd.rf1 = f1;
            double sum = 0.0;
            for (int t = w[0]; t <= w[1]; t++) {
                float v = 0.f;
                if (t >= f0) v = rf.data[std::min(t, f1) - f0] * 1.f;
                if (t >= f0) v = v * tww[t - w[0]];
                reft.push_back(v);
                sum += (double)v * (double)v;                                                      // l2norm, :580
            }
            tw.insert(tw.end(), tww.begin(), tww.end());
            norm_h.push_back(1.f * (float)std::sqrt((double)dt * sum));                            // :589
            comps.push_back(cd);
        }
    }
    recfirst.push_back((int)comps.size());
    const int nmis = (int)comps.size(), nrec_en = (int)recfirst.size() - 1;
    const size_t syn_stride = synofs;
    if (nmis == 0) throw std::runtime_error("no enabled receiver components");
    if (in.has("expect_window")) {           // the recorded set-up's numbers (tests/test_family_fuzz.py): span, halo, wbeg, wlen of receiver 1
        const std::vector<int> e = in.i32("expect_window");
        AUDIT(rec_win[0] == e[0] && rec_win[1] == e[1] && halo == e[2] && rd[0].wbeg == e[3] && rd[0].wlen == e[4],
              "window of receiver 1: span (%d, %d) halo %d wbeg %d wlen %d", rec_win[0], rec_win[1], halo, rd[0].wbeg, rd[0].wlen);
    }
    Buf<RecvDev> recv_d;
    Buf<CompDev> comps_d;
    Buf<float> reft_d, tw_d;
    recv_d.alloc("recv", rd.size()); comps_d.alloc("comps", comps.size()); reft_d.alloc("reft", reft.size()); tw_d.alloc("tw", tw.size());
    std::memcpy(recv_d.p, rd.data(), rd.size() * sizeof(RecvDev));
    std::memcpy(comps_d.p, comps.data(), comps.size() * sizeof(CompDev));
    std::memcpy(reft_d.p, reft.data(), (g_short == "reft" ? reft.size() - 1 : reft.size()) * sizeof(float));
    std::memcpy(tw_d.p, tw.data(), (g_short == "tw" ? tw.size() - 1 : tw.size()) * sizeof(float));

    // ---- run_chunk(c, 0, nsrc, proc_which = 2), kiwi_hip.hip:1078-1212 -- one chunk: the cases are far below KIWI_HIP_CHUNK_MB
    const int cbeg = cent_ofs[0], cend_all = cent_ofs[nsrc];
    int maxnc = 0;
    for (int s = 0; s < nsrc; s++) maxnc = std::max(maxnc, cent_ofs[s + 1] - cent_ofs[s]);
    const size_t nrecords = (size_t)(cend_all - cbeg) * nrec;
    Buf<float> cent_d, moment_d, risetime_d;
    Buf<int> centofs_d;
    cent_d.alloc("cent", std::max<size_t>(cent.size() / 10, 1) * 10); centofs_d.alloc("centofs", (size_t)nsrc + 1);      // :2277-2280
    moment_d.alloc("moment", (size_t)nsrc); risetime_d.alloc("risetime", (size_t)nsrc);
    if (!cent.empty()) std::memcpy(cent_d.p, cent.data(), cent.size() * sizeof(float));
    std::memcpy(centofs_d.p, cent_ofs.data(), cent_ofs.size() * sizeof(int));
    std::memcpy(moment_d.p, moment.data(), moment.size() * sizeof(float));
    std::memcpy(risetime_d.p, risetime.data(), risetime.size() * sizeof(float));
    Buf<GeoRec> recs_d;
    Buf<int> tab_d, off4_d, pairflag_d;
    Buf<float> coef_d;
    recs_d.alloc("recs", nrecords);                                                               // :1084
    tab_d.alloc("tab", nrecords * 128);                                                           // :1088
    const bool compact = db_simple;                                                               // :1089 (c->compact = 1)
    if (compact) { off4_d.alloc("off4", nrecords * 4); off4_d.fill_bytes(0x7f); }
    tab_d.fill_bytes(0x7f);
    coef_d.alloc("coef", nrecords * kCoefLine + 160);                                             // :1096
    coef_d.fill_bytes(0x7f);
    Buf<float> syn_d, proc_d;
    syn_d.alloc("syn", (size_t)nsrc * syn_stride);                                                // :1142 (no fused comparator: proc_which != 0)
    proc_d.alloc("proc", (size_t)nsrc * syn_stride);                                              // :1144
    const bool cell = bilinear && points_per_centroid > 0.5;                                      // :1148 (cell_mode < 0, accum_mode 0)
    const bool duo_maybe = !cell && max_wlen >= 128 && nsrc >= 2;                                 // :1150 (c->duo = 4)
    const EvalParams ep{ bilinear, xus, zus, nrec, 0, cell ? 1 : 0, gaps ? 0 : 1 };              // :1151
    if (maxnc > 0) {
        const dim3 grid((unsigned)((maxnc * nrec + 255) / 256), (unsigned)nsrc);                  // :1162
        if (cell || duo_maybe) {
            pairflag_d.alloc("pairflag", (size_t)nsrc * nrec);                                    // :1164-1165
            for (size_t i = 0; i + (g_short == "pairflag" ? 1 : 0) < (size_t)nsrc * nrec; i++) pairflag_d.p[i] = 0;
        }
        int *pairflag = (cell || duo_maybe) ? pairflag_d.p : nullptr;
        ex.launch(grid, dim3(256), [&] {                                                          // :1176-1178
            geometry_kernel(cent_d.p, centofs_d.p, ep, gm, span.p, recv_d.p, recs_d.p, tab_d.p, coef_d.p, (int *)nullptr, (int *)nullptr, pairflag,
                            endz.p, (const int *)nullptr, (int *)nullptr, (const int *)nullptr, (int4 *)off4_d.p);
        });
        if (cell)                                                                                 // :1179-1182 (c->cell_wave = 1: kCellwRange, kiwi_accum.inc:2483)
            ex.launch(grid, dim3(256), [&] {
                cellgroup_kernel(centofs_d.p, ep, gm, span.p, recv_d.p, recs_d.p, tab_d.p, coef_d.p, pairflag_d.p, endz.p, (const int *)nullptr, 11,
                                 off4_d.p ? 1 : 0);
            });
    }

    // ---- the audit of accumulate_grouped_kernel's addresses (kiwi_accum.inc:1014-1387) over those tables
    const int T = max_wlen >= 2048 ? 256 : (max_wlen >= 384 ? 128 : 64);                          // kiwi_hip.hip:1210
    const int ntiles = (max_wlen + 4 * T - 1) / (4 * T);                                          // :1211
    AuditCount ac;
    {
        const int TILE = 4 * T, LDS_TILE = TILE + kHalo;                                          // kiwi_accum.inc:1033-1034
        const int NG = ng;
        const long long gsize = (long long)G.n;
        const int pairsel = cell ? 1 : 0;                                                         // kiwi_hip.hip:1369 (pairsel 3: the pairs the multi kernel takes are walked here as well)
        for (int s = 0; s < nsrc; s++)
            for (int r = 0; r < nrec; r++)
                for (int tile = 0; tile < ntiles; tile++) {
                    const RecvDev &rv = rd[r];
                    if (!rv.enabled) continue;                                                    // :1048
                    if (tile * TILE >= rv.wlen) continue;                                         // :1049
                    if (pairsel == 1 && rv.need_h && rv.has_d && !(pairflag_d.p[(size_t)s * nrec + r] & 3)) continue;      // :1050, cell_pair()
                    ac.tiles++;
                    const int t_tile0 = rv.wbeg + tile * TILE;                                    // :1055
                    const int c0 = cent_ofs[s], nc = cent_ofs[s + 1] - c0;                        // :1056
                    const size_t rbase = (size_t)(c0 - cbeg) * nrec + (size_t)r * nc;             // :1057-1058
                    const GeoRec *rc = recs_d.p + rbase;
                    const bool need_h = rv.need_h != 0, has_d = rv.has_d != 0;
                    int c = 0;
                    while (c < nc) {                                                              // :1116
                        AUDIT(rbase + c < recs_d.n, "record %d of source %d receiver %d", c, s, r);
                        const GeoRec g0 = rc[c];
                        if (g0.row[0] < 0) { c++; ac.skipped_records++; continue; }               // :1119-1126 (the row prefetched at c + 1 is inside tab: c + 1 < nc)
                        // the group's descriptor row, lane-distributed: ta = lanes 0 .. 63 of the row's first half, tb of its second (:1108,1124,1269)
                        int ta[64], tb[64];
                        if (compact) {                                                            // off4_load + desc_expand, :245-271
                            const int *o = off4_d.p + (rbase + c) * 4;
                            for (int k = 0; k < 4; k++) AUDIT(o[k] != kTabSentinel, "compact descriptor of group start %d (source %d receiver %d) was never written", c, s, r);
                            for (int lane = 0; lane < 64; lane++) {
                                const int fl = (g0.row[lane & 3] - g0.row[0] + (lane >> 2)) * pitch;
                                tb[lane] = fl;
                                ta[lane] = lane < 40 ? fl + o[lane & 3] : 0x7fffffff;
                            }
                        } else {
                            const int *row = tab_d.p + (rbase + c) * 128;
                            AUDIT((rbase + c) * 128 + 128 <= tab_d.n, "descriptor row %d outside tab", c);
                            for (int lane = 0; lane < 64; lane++) { ta[lane] = row[lane]; tb[lane] = row[64 + lane]; }
                            for (int lane = 0; lane < 4 * NG; lane++)
                                AUDIT(ta[lane] != kTabSentinel && tb[lane] != kTabSentinel,
                                      "descriptor row of group start %d (source %d receiver %d tile %d) was never written: lane %d", c, s, r, tile, lane);
                            for (int lane = 40; lane < 52; lane++) AUDIT(ta[lane] != kTabSentinel, "end indices of group start %d (source %d receiver %d) were never written", c, s, r);
                        }
                        const int len = g0.pad & 0xff;
                        const int cend = c + len;                                                 // :1129
                        AUDIT(len >= 1 && cend <= nc, "group at %d of source %d receiver %d: length %d of %d centroids", c, s, r, len, nc);
                        const int smax = g0.ishift + ((g0.pad >> 8) & 0xff), smin = g0.ishift - ((g0.pad >> 16) & 0xff);       // :1130
                        const int jb = t_tile0 - smax - 1;                                        // :1132
                        const int npos = TILE + (smax - smin) + 8;                                // :1133
                        AUDIT(npos <= LDS_TILE, "npos %d of group %d (source %d receiver %d)", npos, c, s, r);
                        const bool direct = (g0.flags & 1) != 0;                                  // :1134
                        const int nk = direct ? 1 : 4;
                        const long long gg = (long long)g0.row[0] * (long long)pitch;             // :1166
                        for (int lane = 0; lane < 4 * NG; lane++)
                            AUDIT(tb[lane] >= 0, "relative floor %d of lane %d, group %d source %d receiver %d (rows %d %d %d %d)", tb[lane], lane, c, s, r,
                                  g0.row[0], g0.row[1], g0.row[2], g0.row[3]);
                        bool fast = true;                                                         // :1169-1170
                        for (int lane = 0; lane < 4 * NG; lane++) fast = fast && (ta[lane] + jb >= tb[lane] && ta[lane] + jb + LDS_TILE <= tb[lane] + pitch);
                        auto load4 = [&](long long idx, const char *what, int ig, int k, int lanepos) {      // a 16-byte load at Gg + idx
                            ac.loads++;
                            AUDIT(gg + idx >= 0 && gg + idx + 4 <= gsize, "%s of component %d node %d position %d reads G[%lld .. +4) of %lld: group %d source %d receiver %d tile %d",
                                  what, ig, k, lanepos, gg + idx, gsize, c, s, r, tile);
                        };
                        // main loads: LDS positions [4 tid, 4 tid + 4) of every component built (build_batch :300-333, pair_issue :338-357)
                        std::vector<int> igs;
                        if (need_h && has_d) for (int ig = 0; ig < NG; ig++) igs.push_back(ig);    // :1233
                        else if (need_h) igs = NG == 10 ? std::vector<int>{ 0, 1, 2, 3, 4, 8 } : std::vector<int>{ 0, 1, 2, 3, 4 };      // :1183-1184, 1253-1256
                        else igs = NG == 10 ? std::vector<int>{ 5, 6, 7, 9 } : std::vector<int>{ 5, 6, 7 };
                        for (int tid = 0; tid < T; tid++) {
                            const int p = 4 * tid, j = jb + p;
                            for (int ig : igs)
                                for (int k = 0; k < nk; k++) {
                                    const int base = ta[4 * ig + k];
                                    if (fast) {                                                    // buf_load4(rsrc, p, base + jb): both offsets unsigned (:55-61)
                                        AUDIT(base + jb >= 0, "fast load with a negative row offset %d", base + jb);
                                        load4((long long)p + (long long)(base + jb), "fast main load", ig, k, p);
                                    } else {                                                       // :314-316, 351-353
                                        const int lo = tb[4 * ig + k];
                                        const int idx = std::min(std::max(base + j, lo), lo + pitch - 4);
                                        load4((long long)(unsigned)idx, "main load", ig, k, p);
                                    }
                                }
                        }
                        // halo loads: halo_lane :1198-1209, halo_issue :417-433; passes :1190-1191, 1210, 1226
                        const int kHaloIter = (16 * NG + T - 1) / T;
                        const bool chunk_major = T < 256;
                        const int ncmp = (need_h && has_d) ? NG : (need_h ? (NG == 10 ? 6 : 5) : (NG == 10 ? 4 : 3));
                        for (int it = 0; it < kHaloIter; it++) {
                            const bool first = chunk_major ? it == 0 : true;                      // passes in flight with the main loads: take the `fast` form
                            if (!first && !(4 * ((it * T) / ncmp) < npos - TILE)) break;
                            for (int tid = 0; tid < T; tid++) {
                                const int q = tid + it * T;
                                const int slot = chunk_major ? q % ncmp : q >> 4, chunk = chunk_major ? q / ncmp : q & 15;
                                int ig = slot;
                                if (!(need_h && has_d)) {
                                    if (need_h) ig = (slot == 5) ? 8 : slot;
                                    else ig = (NG == 10 && slot == 3) ? 9 : 5 + slot;
                                }
                                ig = std::min(ig, NG - 1);
                                const int ph = TILE + 4 * std::min(chunk, 15);
                                if (!(slot < ncmp && chunk < 16 && ph < npos)) continue;
                                AUDIT(ph + 4 <= LDS_TILE && ig * LDS_TILE + ph + 4 <= NG * LDS_TILE, "halo store at LDS position %d of component %d", ph, ig);
                                for (int k = 0; k < nk; k++) {
                                    const int base = ta[4 * ig + k];
                                    int idx = base + jb + ph;
                                    if (!(first && fast)) { const int lo = tb[4 * ig + k]; idx = std::min(std::max(idx, lo), lo + pitch - 4); }
                                    load4((long long)(unsigned)idx, "halo load", ig, k, ph);
                                }
                            }
                        }
                        // apply: every centroid of the group reads b[j-1], b[j] at e + u0 + 64 q (+ 1), q = 0 .. 3 (:1362-1364, tile_load :519-529)
                        const int u0max = 4 * ((T - 1) & ~63) + 63;
                        for (int cc = c; cc < cend; cc++) {
                            AUDIT(rc[cc].row[0] >= 0, "centroid %d inside the group at %d is a skipped one", cc, c);
                            const int e = smax - rc[cc].ishift;
                            AUDIT(e >= 0 && e + u0max + 193 < LDS_TILE && e + u0max + 193 < npos, "apply of centroid %d: e = %d, group %d source %d receiver %d", cc, e, c, s, r);
                            const unsigned *cl = (const unsigned *)(coef_d.p + (rbase + cc) * kCoefLine);      // :1350-1361
                            AUDIT((rbase + cc) * kCoefLine + 2 * NG <= coef_d.n, "coefficient line %d outside coef", cc);
                            for (int i = 0; i < 2 * NG; i++) AUDIT(cl[i] != kCoefSentinel, "coefficient line of centroid %d (source %d receiver %d) was never written", cc, s, r);
                            ac.applies++;
                        }
                        ac.groups++;
                        c = cend;                                                                 // :1379
                    }
                    // the store, :1064-1083: samples tl + 64 i < wlen of every component into the source's slot of syn
                    for (int tid = 0; tid < T; tid++) {
                        const int tl = tile * TILE + 4 * (tid & ~63) + (tid & 63);
                        if (tl >= rv.wlen) continue;
                        for (int k = 0; k < rv.ncomp; k++)
                            for (int i = 0; i < 4; i++)
                                if (tl + 64 * i < rv.wlen) {
                                    const long long at = (long long)rv.synofs[k] + tl + 64 * i;
                                    ac.stores++;
                                    AUDIT(at >= 0 && at < (long long)syn_stride && (size_t)s * syn_stride + (size_t)at < syn_d.n,
                                          "store at %lld of a slot of %zu: source %d receiver %d component %d", at, syn_stride, s, r, k);
                                }
                    }
                }
    }

    // ---- what the accumulate kernel leaves in syn_d: the oracle's plain strips over each window -- zeros in front of a strip, its
    // last value behind it (every centroid's trace is held at its end value: sparse_trace.f90:698-703)
    {
        const std::vector<int> sfirst = in.i32("strip_first"), sofs = in.i32("strip_ofs");
        const std::vector<float> sdata = in.f32("strip_data");
        if ((int)sofs.size() != nsrc * nmis + 1) throw std::runtime_error("strips do not fit the slots");
        for (size_t i = 0; i + (g_short == "syn" ? 1 : 0) < syn_d.n; i++) syn_d.p[i] = 0.f;
        for (int s = 0; s < nsrc; s++)
            for (int m = 0; m < nmis; m++) {
                const CompDev &cd = comps[m];
                const RecvDev &rv = rd[cd.rec];
                const int q = s * nmis + m, n = sofs[q + 1] - sofs[q], f0 = sfirst[q];
                float *row = syn_d.p + (size_t)s * syn_stride + cd.synofs;
                for (int i = 0; i < rv.wlen; i++) {
                    const int t = rv.wbeg + i;
                    row[i] = (n > 0 && t >= f0) ? sdata[(size_t)sofs[q] + std::min(t - f0, n - 1)] : 0.f;
                }
            }
    }

    // ---- misfit_kernel with `proc`, kiwi_hip.hip:1390-1453 (l2norm, proc_which 2: the tapered traces are kept)
    Buf<float> misfit_d;
    misfit_d.alloc("misfit", (size_t)nsrc * nmis);                                                // kiwi_linfit.hpp run(): misfit_d.ensure
    {
        MisfitParams mp{ 1, dt, syn_factor, nmis, 0, 2, 0, nsrc, 0 };
        ex.launch(dim3((unsigned)nmis, (unsigned)nsrc), dim3(256), [&] {
            misfit_kernel(syn_d.p, syn_stride, comps_d.p, reft_d.p, tw_d.p, moment_d.p, risetime_d.p, mp, misfit_d.p, proc_d.p, (float *)nullptr, (float *)nullptr,
                          (const int *)nullptr, (const FftPair *)nullptr, (const int *)nullptr);
        });
    }
    // ---- global_kernel, kiwi_hip.hip:1502-1505 (no rejected source, no transform: status and norm_src are null)
    Buf<float> norm_d, global_d;
    Buf<int> recfirst_d;
    norm_d.alloc("norm", norm_h.size()); recfirst_d.alloc("recfirst", recfirst.size()); global_d.alloc("global", (size_t)nsrc);
    std::memcpy(norm_d.p, norm_h.data(), norm_h.size() * sizeof(float));
    std::memcpy(recfirst_d.p, recfirst.data(), recfirst.size() * sizeof(int));
    ex.launch(dim3((unsigned)((nsrc + 127) / 128)), dim3(128), [&] {
        global_kernel(misfit_d.p, norm_d.p, recfirst_d.p, nrec_en, nmis, 0, nsrc, global_d.p, (const int *)nullptr, (const float *)nullptr);
    });
    if (in.has("proc_rows")) {               // the kept traces of another run (a device's) in place of these: [slot][source][wlen of the slot]
        const std::vector<float> rows = in.f32("proc_rows");
        size_t at = 0;
        for (int m = 0; m < nmis; m++)
            for (int s = 0; s < nsrc; s++) {
                std::memcpy(proc_d.p + (size_t)s * syn_stride + comps[m].synofs + comps[m].halo, rows.data() + at, (size_t)comps[m].wlen * sizeof(float));
                at += (size_t)comps[m].wlen;
            }
        if (at != rows.size()) throw std::runtime_error("proc_rows do not fit the slots");
    }

    // ---- linfit_gram_kernel<K>, linfit_solve_kernel<K>: kiwi_linfit.hpp run() / launch_gram / launch
    const int NN = linfit::nn_of(K);
    std::vector<double> w((size_t)nrec, 0.0);                                                     // kiwi_group_run.hpp receiver_weights
    {
        const std::vector<double> given = in.has("weights") ? in.f64("weights") : std::vector<double>();
        for (int r = 0; r < nrec; r++) if (recv[r].enabled && recv[r].ncomp > 0) w[r] = given.empty() ? 1.0 : given[r];
    }
    Buf<double> w_d, nbr_d, coefx_d, mis_d, piv_d, normal_d;
    Buf<int> st_d;
    w_d.alloc("w", (size_t)nrec);
    std::memcpy(w_d.p, w.data(), (size_t)nrec * sizeof(double));
    nbr_d.alloc("nbr", (size_t)ngroup * nrec * NN);
    coefx_d.alloc("coefx", (size_t)ngroup * K); mis_d.alloc("mis", (size_t)ngroup); piv_d.alloc("piv", (size_t)ngroup); st_d.alloc("st", (size_t)ngroup);
    normal_d.alloc("normal", (size_t)ngroup * NN);
    for (size_t i = 0; i + (g_short == "nbr" ? 1 : 0) < nbr_d.n; i++) nbr_d.p[i] = 0.0;          // hipMemsetAsync(nbr_d)
    by_basis(K, [&](auto k) {
        constexpr int KK = decltype(k)::value;
        ex.launch(dim3((unsigned)nrec, (unsigned)ngroup), dim3(linfit::kThreads), [&] {
            linfit::linfit_gram_kernel<KK>(proc_d.p, syn_stride, recv_d.p, comps_d.p, reft_d.p, (const float *)nullptr, (const FftPair *)nullptr, nmis, nrec,
                                           syn_factor, dt, nbr_d.p);
        });
        ex.launch(dim3((unsigned)((ngroup + 63) / 64)), dim3(64), [&] {
            linfit::linfit_solve_kernel<KK>(nbr_d.p, w_d.p, nrec, anarchy, ngroup, coefx_d.p, mis_d.p, st_d.p, piv_d.p, normal_d.p);
        });
    });

    // ---- results
    out.put("layout", std::vector<int>{ halo, max_wlen, T, ntiles, (int)syn_stride, cell ? 1 : 0, compact ? 1 : 0, nmis, pitch, gaps ? 1 : 0, nsrc, ngroup });
    out.put("rec_win", rec_win);
    out.put("recs", 0, (const int *)recs_d.p, recs_d.n * 20);
    out.put("cent_ofs", cent_ofs);
    out.put("misfit", 1, misfit_d.p, misfit_d.n);
    out.put("norm", norm_h);
    out.put("global", 1, global_d.p, global_d.n);
    {
        std::vector<float> rows, refs;
        std::vector<int> wl;
        for (int m = 0; m < nmis; m++) {
            wl.push_back(comps[m].wlen);
            refs.insert(refs.end(), reft.begin() + comps[m].refofs, reft.begin() + comps[m].refofs + comps[m].wlen);
            for (int s = 0; s < nsrc; s++) {
                const float *p = proc_d.p + (size_t)s * syn_stride + comps[m].synofs + comps[m].halo;
                rows.insert(rows.end(), p, p + comps[m].wlen);
            }
        }
        out.put("slot_wlen", wl); out.put("proc", rows); out.put("reft", refs);
    }
    out.put("by_receiver", 2, nbr_d.p, nbr_d.n);
    out.put("normal", 2, normal_d.p, normal_d.n);
    out.put("coef", 2, coefx_d.p, coefx_d.n);
    out.put("fit_misfit", 2, mis_d.p, mis_d.n);
    out.put("status", 0, st_d.p, st_d.n);
    out.put("pivot_min", 2, piv_d.p, piv_d.n);
    out.put("audit", std::vector<double>{ (double)ac.tiles, (double)ac.groups, (double)ac.loads, (double)ac.stores, (double)ac.applies, (double)ac.skipped_records });
    out.write(argv[2]);
    std::printf("linfit path host run: clean (%s%s, T = %d, %d tile%s, halo %d; %llu launches, %llu workgroups, %llu rendezvous; audit: %lld tiles, %lld groups, %lld loads, %lld stores)\n",
                cell ? "cell mode" : "same-point groups", compact ? ", compact descriptors" : "", T, ntiles, ntiles == 1 ? "" : "s", halo, ex.launches, ex.groups_run,
                (unsigned long long)ex.rendezvous, ac.tiles, ac.groups, ac.loads, ac.stores);
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    try {
        return run(argc, argv);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "linfit_path_host: %s\n", e.what());
        return 3;
    }
}
