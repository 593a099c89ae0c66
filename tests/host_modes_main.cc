// Host check of the switch table's parse functions (juicefs_amd/csrc/host_modes.h),
// built with AddressSanitizer and UBSan by tests/test_modes.py: every documented
// spelling in three cases, what is no spelling, a null pointer, an empty string
// and a 4 KiB string, for every switch of the table.  Prints "ok <checks>".
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "host_modes.h"

using namespace jfs_host;

static int g_checks = 0, g_bad = 0;

static void expect(const char *what, const char *s, long long got, long long want) {
    g_checks++;
    if (got == want) return;
    g_bad++;
    printf("FAIL %s \"%.40s\": got %lld, want %lld\n", what, s ? s : "(null)", got, want);
}

// heap copies of exactly the string's size, so that a read past its end is caught
static void mode_is(const ModeDesc &d, const std::string &s, int want) {
    std::vector<char> heap(s.c_str(), s.c_str() + s.size() + 1);
    expect(d.env, heap.data(), mode_parse(d, heap.data()), want);
}
static void int_is(const IntDesc &d, const std::string &s, int64_t want) {
    std::vector<char> heap(s.c_str(), s.c_str() + s.size() + 1);
    expect(d.env, heap.data(), int_parse(d, heap.data()), want);
}

static std::string mixed(std::string w) {
    for (size_t i = 1; i < w.size(); i += 2) w[i] = (char)toupper((unsigned char)w[i]);
    return w;
}
static std::string upper(std::string w) {
    for (char &c : w) c = (char)toupper((unsigned char)c);
    return w;
}

static void check_mode(const ModeDesc &d) {
    int nwords = 0;
    for (const ModeWord &w : d.words) {
        if (!w.word) continue;
        nwords++;
        const std::string s(w.word);
        mode_is(d, s, w.value);
        mode_is(d, upper(s), w.value);
        mode_is(d, mixed(s), w.value);
        mode_is(d, s + "x", d.def);                   // no prefix match
        mode_is(d, s.substr(0, s.size() - 1), d.def);  // nor the other way round
        mode_is(d, " " + s, d.def);
        expect(d.env, "value in range", w.value >= 0 && w.value <= d.ext_max, 1);
    }
    expect(d.env, "words", nwords, d.ext_max + 1);
    expect(d.env, "setters", d.set_max >= 0 && d.set_max <= d.ext_max, 1);
    expect(d.env, nullptr, mode_parse(d, nullptr), d.def);
    mode_is(d, "", d.def);
    mode_is(d, "bogus", d.def);
    mode_is(d, "1", d.def);
    mode_is(d, std::string(4096, 'o'), d.def);
    mode_is(d, std::string(d.words[1].word) + std::string(4096, ' '), d.def);
}

static void check_int(const IntDesc &d) {
    expect(d.env, nullptr, int_parse(d, nullptr), d.def);
    int_is(d, "", d.def);
    int_is(d, "bogus", d.def);
    int_is(d, "1", 1);
    int_is(d, std::to_string(d.lo), d.lo);
    int_is(d, std::to_string(d.hi), d.hi);
    int_is(d, std::to_string(d.lo - 1), d.def);
    int_is(d, std::to_string(d.hi + 1), d.def);
    int_is(d, "12abc", d.def);
    int_is(d, "12 ", d.def);
    int_is(d, "99999999999999999999999999", d.def);
    int_is(d, "-99999999999999999999999999", d.def);
    int_is(d, std::string(4096, '7'), d.def);
    int_is(d, std::string(4095, '0') + "1", 1);
}

int main() {
    for (const ModeDesc *d : {&MODE_LZ4_PARSE, &MODE_READ_DECODE, &MODE_READ_SEEK, &MODE_READ_LZ4_CHASE, &MODE_ZSTD_PARSE,
                              &MODE_ZSTD_SEEK_CSUM, &MODE_COMPACT_SPLICE})
        check_mode(*d);
    check_int(INT_LZ4_CHASE_MAX);
    check_int(INT_ZSTD_SPLIT_FRAMES);
    // the spellings of include/jfs_gpucodec.h, once by hand
    expect("JFS_READ_DECODE", "PREFIX-ALL", mode_parse(MODE_READ_DECODE, "PREFIX-ALL"), JFS_READ_DECODE_PREFIX_ALL);
    expect("JFS_READ_SEEK", "Sparse", mode_parse(MODE_READ_SEEK, "Sparse"), JFS_READ_SEEK_SPARSE);
    expect("JFS_ZSTD_PARSE", "seekable", mode_parse(MODE_ZSTD_PARSE, "seekable"), JFS_ZSTD_PARSE_SEEKABLE);
    expect("JFS_COMPACT_SPLICE", "ALL", mode_parse(MODE_COMPACT_SPLICE, "ALL"), JFS_COMPACT_SPLICE_ALL);
    expect("JFS_LZ4_PARSE", "fast", mode_parse(MODE_LZ4_PARSE, "fast"), JFS_LZ4_PARSE_FAST);
    if (g_bad) return 1;
    printf("ok %d\n", g_checks);
    return 0;
}
