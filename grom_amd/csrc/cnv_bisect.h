// cnv_bisect.h -- the reference's three bisects (GROM.c:21630-21860, exact,
// off-by-one exits included), one definition for the kernels (cnv.hip) and
// the host math (cnvcall.cpp).
#pragma once

#if defined(__HIPCC__)
#define CNV_HD __host__ __device__
#else
#define CNV_HD
#endif

static CNV_HD long cnv_bisect_left(const int *l, int rd, long s, long e) {
    int found = 0;
    long i = s + (e - s) / 2, lo = s, hi = e;
    while (found == 0) {
        if (i <= s) { i = (rd <= l[s]) ? s : s + 1; found = 1; }
        else if (i >= e - 1) { i = (rd <= l[e - 1]) ? e - 1 : e; found = 1; }
        else if (rd <= l[i]) { hi = i; i = lo + (i - lo) / 2; if (hi == i) { found = 1; i += 1; } }
        else { lo = i; i = i + (hi - i) / 2; if (lo == i) { found = 1; i += 1; } }
    }
    return i;
}
static CNV_HD long cnv_bisect_right(const int *l, int rd, long s, long e) {
    int found = 0;
    long i = s + (e - s) / 2, lo = s, hi = e;
    while (found == 0) {
        if (i <= s) { i = (rd < l[s]) ? s : s + 1; found = 1; }
        else if (i >= e - 1) { i = (rd < l[e - 1]) ? e - 1 : e; found = 1; }
        else if (rd < l[i]) { hi = i; i = lo + (i - lo) / 2; if (hi == i) { found = 1; i += 1; } }
        else { lo = i; i = i + (hi - i) / 2; if (lo == i) { found = 1; i += 1; } }
    }
    return i;
}
static CNV_HD long cnv_bisect_right_double(const double *l, double p, long s, long e) {
    int found = 0;
    long i = s + (e - s) / 2, lo = s, hi = e;
    while (found == 0) {
        if (i <= s) { i = (p < l[s]) ? s : s + 1; found = 1; }
        else if (i >= e - 1) { i = (p < l[e - 1]) ? e - 1 : e; found = 1; }
        else if (p < l[i]) { hi = i; i = lo + (i - lo) / 2; if (hi == i) { found = 1; i += 1; } }
        else { lo = i; i = i + (hi - i) / 2; if (lo == i) { found = 1; i += 1; } }
    }
    return i;
}
