// HITRAN .par records on the host: the validity rule of include/clearsky_hip.h (cs_par_parse) in one place.  Plain C++17, no HIP and no
// library state in here, so that the file compiles into a stand-alone program (a sanitizer build, a timing loop) as it stands.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <locale.h>
#include <string>
#include <thread>
#include <vector>

namespace cs_par {

constexpr size_t RECORD = 160;   // characters of a record (par.jl:131-149), terminator not counted

// the numeric fields in file order: columns a..b (1-based, inclusive), like parse(Float64, line[a:b]) at par.jl:133-140
struct Field {
    const char *name;
    int a, b;
};
constexpr Field FIELDS[8] = {{"nu", 4, 15},      {"S", 16, 25},   {"A", 26, 35},  {"gamma_a", 36, 40},
                             {"gamma_s", 41, 45}, {"Epp", 46, 55}, {"na", 56, 59}, {"delta_a", 60, 67}};

struct Arrays {   // the caller's arrays of cs_par_parse
    int16_t *M;
    char *I;
    double *v[8];   // in the order of FIELDS
};

inline bool is_space(char c) { return c == ' ' || (c >= '\t' && c <= '\r'); }
inline bool is_digit(char c) { return c >= '0' && c <= '9'; }

// ISOINDEX, par.jl:6-13: '1'..'9' -> 1..9, '0' -> 10, 'A'..'Z' -> 11..36; 0 = not an isotopologue character
inline int iso_index(char c)
{
    if (c >= '1' && c <= '9') return c - '0';
    if (c == '0') return 10;
    if (c >= 'A' && c <= 'Z') return 11 + (c - 'A');
    return 0;
}

// The "C" locale, made once: strtod_l reads by it whatever LC_NUMERIC the host application has set (under a decimal-comma locale plain
// strtod stops at the point and returns the integer part of every field).  No comma locale is installed where the suite runs, so no
// test covers this; the call below is the whole of the property.
inline locale_t c_locale()
{
    static const locale_t loc = newlocale(LC_ALL_MASK, "C", (locale_t)0);
    return loc;
}

inline void trim(const char *&s, int &w)
{
    while (w && *s == ' ') s++, w--;
    while (w && s[w - 1] == ' ') w--;
}

// A field of w characters: blanks trimmed on both sides, the whole remainder a plain decimal literal -- optional sign, digits with an
// optional point (at least one digit), optional e/E exponent with optional sign and at least one digit -- and its value finite.  The
// grammar is checked here, so the hex floats, "nan", "inf" and partial reads strtod would accept never reach it.  Correctly rounded:
// the digits m (at most 15 in these columns, so m < 2^53) and a power of ten up to 10^22 are both exact in fp64, and m * 10^k or
// m / 10^k is then one rounded operation (Clinger's fast path; most fields of a record take it); the others -- an intensity of 1e-30
// -- go to glibc's strtod, which rounds correctly, subnormals included.
inline bool decimal(const char *s, int w, locale_t loc, double &out)
{
    static const double P10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                   1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    trim(s, w);
    int i = 0, nd = 0, ne = 0, nfrac = 0, ex = 0;
    uint64_t m = 0;
    const bool neg = w && s[0] == '-';
    if (i < w && (s[i] == '+' || s[i] == '-')) i++;
    for (; i < w && is_digit(s[i]); i++, nd++) m = 10 * m + (uint64_t)(s[i] - '0');
    if (i < w && s[i] == '.')
        for (i++; i < w && is_digit(s[i]); i++, nd++, nfrac++) m = 10 * m + (uint64_t)(s[i] - '0');
    if (!nd) return false;
    if (i < w && (s[i] == 'e' || s[i] == 'E')) {
        i++;
        const bool eneg = i < w && s[i] == '-';
        if (i < w && (s[i] == '+' || s[i] == '-')) i++;
        for (; i < w && is_digit(s[i]); i++, ne++) ex = std::min(10 * ex + (s[i] - '0'), 100000);
        if (!ne) return false;
        if (eneg) ex = -ex;
    }
    if (i != w || w > 15) return false;
    const int k = ex - nfrac;
    if (m == 0 || (k >= -22 && k <= 22)) {
        const double v = m == 0 ? 0.0 : k < 0 ? (double)m / P10[-k] : (double)m * P10[k];
        out = neg ? -v : v;
        return true;
    }
    char buf[16];
    memcpy(buf, s, (size_t)w);
    buf[w] = 0;
    out = strtod_l(buf, nullptr, loc);
    return std::isfinite(out);
}

// columns 1-2: blanks trimmed, optional sign, digits, nothing else
inline bool integer(const char *s, int w, int16_t &out)
{
    trim(s, w);
    int i = 0, v = 0;
    const bool neg = w && s[0] == '-';
    if (i < w && (s[i] == '+' || s[i] == '-')) i++;
    if (i == w) return false;
    for (; i < w; i++) {
        if (!is_digit(s[i])) return false;
        v = 10 * v + (s[i] - '0');
    }
    out = (int16_t)(neg ? -v : v);
    return true;
}

// Record i of the file into element i of the arrays; the name of the first field (in file order) that breaks the rule, or nullptr.
inline const char *parse_record(const char *r, int64_t i, const Arrays &o, locale_t loc)
{
    if (!integer(r, 2, o.M[i])) return "M";
    if (!iso_index(r[2])) return "I";
    o.I[i] = r[2];
    for (int q = 0; q < 8; q++)
        if (!decimal(r + FIELDS[q].a - 1, FIELDS[q].b - FIELDS[q].a + 1, loc, o.v[q][i])) return FIELDS[q].name;
    return nullptr;
}

// The layout pass: offsets of the records of p[0 .. len).  A record ends at LF, one CR directly before that LF belongs to the terminator
// (decided record by record); the last record may lack a terminator; lines of whitespace only are allowed at the very end of the file.
// Every record has RECORD characters: anything else is refused with its 1-based number and the length found.
inline bool index_records(const char *p, size_t len, std::vector<size_t> &off, std::string &err)
{
    off.clear();
    off.reserve(len / (RECORD + 1) + 1);
    size_t pos = 0;
    while (pos < len) {
        const char *nl = (const char *)memchr(p + pos, '\n', len - pos);
        const size_t end = nl ? (size_t)(nl - p) : len;
        size_t body = end - pos;
        if (nl && body && p[end - 1] == '\r') body--;
        if (body != RECORD) {
            size_t q = pos;
            while (q < len && is_space(p[q])) q++;
            if (q == len) break;   // blank lines at the end of the file
            char buf[160];
            snprintf(buf, sizeof buf, "record %lld has %zu characters, a HITRAN .par record has %zu", (long long)off.size() + 1, body, RECORD);
            err = buf;
            return false;
        }
        off.push_back(pos);
        pos = end + 1;
    }
    if (off.empty()) {
        err = "the file holds no records";
        return false;
    }
    return true;
}

inline int thread_count(int64_t n)
{
    return (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)std::thread::hardware_concurrency(), 32, n / 20000}));
}

// All records into the arrays, on thread_count(n) threads over contiguous shares.  Each thread stops at the first record of its share
// that breaks the rule; the lowest such record of the file is the one reported, whichever thread found it.  On refusal the arrays hold
// unspecified values in elements 0 .. n-1 (every thread has written what it got to) and nothing outside them.
inline bool parse_records(const char *p, const std::vector<size_t> &off, const Arrays &o, std::string &err)
{
    const int64_t n = (int64_t)off.size();
    const int nth = thread_count(n);
    const locale_t loc = c_locale();
    std::vector<int64_t> bad(nth, -1);
    std::vector<const char *> what(nth, nullptr);
    auto share = [&](int t) {
        for (int64_t i = n * t / nth; i < n * (t + 1) / nth; i++)
            if (const char *f = parse_record(p + off[i], i, o, loc)) {
                bad[t] = i;
                what[t] = f;
                return;
            }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nth; t++) th.emplace_back(share, t);
    share(0);
    for (auto &x : th) x.join();
    for (int t = 0; t < nth; t++) {   // shares ascend with t: the first hit is the lowest record
        if (bad[t] < 0) continue;
        const char *r = p + off[bad[t]];
        const char *f = what[t];
        int a = 1, b = 2;
        if (!strcmp(f, "I")) a = b = 3;
        for (const Field &F : FIELDS)
            if (!strcmp(f, F.name)) a = F.a, b = F.b;
        char txt[16] = {0};
        for (int c = a; c <= b && c - a < 15; c++) txt[c - a] = (r[c - 1] >= ' ' && r[c - 1] < 127) ? r[c - 1] : '?';
        const char *rule = a == 1 ? "an integer literal" : a == 3 ? "an isotopologue character (1-9, 0, A-Z)" : "a finite plain decimal literal";
        char buf[200];
        snprintf(buf, sizeof buf, "record %lld: field %s (columns %d-%d) = '%s' is not %s", (long long)bad[t] + 1, f, a, b, txt, rule);
        err = buf;
        return false;
    }
    return true;
}

}  // namespace cs_par
