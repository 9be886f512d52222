// AddressSanitizer / UBSan run of the staged eikonal discretiser (CPU build only): prepare over a batch, the solve cache's two
// halves around solves done elsewhere -- here: packed into one buffer and marched by the host's routines --, finish; against
// discretize_eikonal, which composes the same three stages per source.
#include "kiwi_host_eikonal.hpp"
#include <cstdio>
#include <random>
using namespace kiwi;
int main()
{
    std::mt19937 rng(424242);
    auto U = [&](float a, float b) { return a + (b - a) * (float)(rng() % 100000) / 100000.f; };
    float crust[31] = { 1500., 3810., 2500., 4000., 6000., 6400., 6900., 8100., 0., 1940., 1200., 2300., 3500., 3700., 3900., 4600., 1020., 920., 2100., 2400., 2750., 2850., 3000., 3350., 0., 0., 1000., 1000., 10000., 10000., 10000. };
    CrustProfile pr; std::memcpy(&pr, crust, sizeof pr);
    std::vector<HalfSpace> cons(2);
    cons[0] = { { 0, 0, 1500.f }, { 0, 0, -1.f } }; cons[1] = { { 0, 0, 31000.f }, { 0, 0, 1.f } };
    int bad = 0, nok = 0, nrej = 0, nhit = 0;
    // the size guard of the int-indexed layouts
    if (!eik::grid_fits_int(1200, 360) || eik::grid_fits_int(1ll << 30, 1) || eik::grid_fits_int(46339, 46339) || !eik::grid_fits_int(46338, 46338) || eik::grid_fits_int(0, 4)) bad++;
    for (int round = 0; round < 6; round++) {
        const int n = 16;
        std::vector<std::array<float, 20>> P((size_t)n);
        std::vector<int> type((size_t)n);
        for (int c = 0; c < n; c++) {
            const int st = 4 + c % 2;
            float *p = P[(size_t)c].data();
            std::fill(p, p + 20, 0.f);
            if (c >= 12) { std::memcpy(p, P[(size_t)c - 12 + (st == type[(size_t)c - 12] ? 0 : 1)].data(), 20 * sizeof(float)); p[1] += 300.f; p[0] += 0.5f; type[(size_t)c] = type[(size_t)c - 12 + (st == type[(size_t)c - 12] ? 0 : 1)]; continue; }   // a shifted copy: the same solve
            type[(size_t)c] = st;
            p[0] = U(-1, 1); p[1] = U(-3e3f, 3e3f); p[2] = U(-3e3f, 3e3f); p[3] = U(2e3f, 3e4f); p[4] = 1.f; p[5] = U(-180, 180); p[6] = U(0, 90);
            const int o = st == 5 ? 0 : 1;
            if (st == 4) p[7] = U(-180, 180);
            p[7 + o] = U(-2e3f, 2e3f); p[8 + o] = U(-2e3f, 2e3f); p[9 + o] = U(5e2f, 7e3f);
            p[10 + o] = U(-1, 1) * 0.9f * p[9 + o]; p[11 + o] = U(-1, 1) * 0.9f * p[9 + o]; p[12 + o] = U(0.5f, 1.f);
            if (st == 5) { for (int k = 0; k < 6; k++) p[13 + k] = U(-1, 1) * 1e18f; p[19] = U(0, 3); } else p[14] = U(0, 3);
            if (c == 5) p[3] = -9e4f;                                   // above the surface: "Empty rupture area"
        }
        const float edt = round % 3 == 0 ? 0.5f : (round % 3 == 1 ? 1.f : 2.f);
        eik::fmm_mode() = round % 2;                                   // both sets of grid passes
        // stage 1 and the cache's first half
        std::vector<EikonalStage> st((size_t)n);
        std::vector<std::string> err((size_t)n);
        std::vector<eik::CacheProbe> probe((size_t)n);
        std::vector<char> need((size_t)n, 0);
        for (int c = 0; c < n; c++) {
            err[(size_t)c] = eikonal_prepare(type[(size_t)c], P[(size_t)c].data(), edt, pr, cons, st[(size_t)c]);
            if (!err[(size_t)c].empty()) continue;
            EikonalStage &q = st[(size_t)c];
            need[(size_t)c] = !eik::solve_cache_lookup(q.speed, q.fx, q.fy, q.lo, q.fd, q.start, q.ftimes, q.invalid, probe[(size_t)c]);
            if (!need[(size_t)c]) nhit++;
        }
        // the solves as a packed batch: offsets, one buffer of speeds, one of times
        std::vector<long long> ofs((size_t)n, 0);
        long long total = 0;
        for (int c = 0; c < n; c++) if (need[(size_t)c]) { ofs[(size_t)c] = total; total += (long long)st[(size_t)c].fx * st[(size_t)c].fy; }
        std::vector<float> speed((size_t)total), times((size_t)total);
        for (int c = 0; c < n; c++) if (need[(size_t)c]) std::memcpy(speed.data() + ofs[(size_t)c], st[(size_t)c].speed.data(), st[(size_t)c].speed.size() * sizeof(float));
        for (int c = 0; c < n; c++) {
            if (!need[(size_t)c]) continue;
            EikonalStage &q = st[(size_t)c];
            std::vector<float> t;
            if (c % 2) eik::fast_marching_plain(speed.data() + ofs[(size_t)c], q.fx, q.fy, q.lo, q.fd, q.start, t, q.invalid);
            else eik::fast_marching(speed.data() + ofs[(size_t)c], q.fx, q.fy, q.lo, q.fd, q.start, t, q.invalid);
            std::memcpy(times.data() + ofs[(size_t)c], t.data(), t.size() * sizeof(float));
        }
        for (int c = 0; c < n; c++) {
            if (!need[(size_t)c]) continue;
            EikonalStage &q = st[(size_t)c];
            q.ftimes.assign(times.begin() + ofs[(size_t)c], times.begin() + ofs[(size_t)c] + (long long)q.fx * q.fy);
            eik::solve_cache_store(q.speed, q.fx, q.fy, q.fd, q.ftimes, probe[(size_t)c]);
        }
        // stage 3, against the un-split function
        for (int c = 0; c < n; c++) {
            DiscreteSource a, b;
            const std::string ea = discretize_eikonal(type[(size_t)c], P[(size_t)c].data(), edt, pr, cons, a);
            const std::string eb = err[(size_t)c].empty() ? eikonal_finish(st[(size_t)c], b) : err[(size_t)c];
            if (ea != eb) { bad++; continue; }
            if (!ea.empty()) { nrej++; continue; }
            nok++;
            if (a.centroids.size() != b.centroids.size() || std::memcmp(a.centroids.data(), b.centroids.data(), a.centroids.size() * sizeof(Centroid))) bad++;
            if (std::memcmp(&a.moment, &b.moment, 4) || std::memcmp(&a.risetime, &b.risetime, 4)) bad++;
        }
    }
    if (nrej < 6 || nok < 40) bad++;
    std::printf("asan staged run: %d bad, %d ruptures discretised, %d rejected, %d answered by the cache before their solve\n", bad, nok, nrej, nhit);
    return bad != 0;
}
