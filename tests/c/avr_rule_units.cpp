/* avr_rule_units.cpp -- the line rule of the AVR text input as the device runs it (msd_avr_impl.h: line_at over a
 * Window's masks, put_record) against the host reader (msd_avr_reader_feed, which tests/test_avr_reader.py holds to the
 * reference's rule), as a stand-alone program so that a sanitizer build can watch the mask code's two-word reads and
 * its guard word (tests/test_avr_rule_units.py builds it with -fsanitize=address,undefined).
 *
 * A case is a piece of bytes laid into a window from position rmin on; every other byte of the window is 0xff and has
 * no class, as classify leaves it.  The masks are filled here, by a plain loop over the class tests classify uses.  For
 * every '\n' at a position r >= LB -- the ones a thread can own -- line_at's answer is compared with what the reader
 * does when it is fed the piece up to and including that '\n': the counter that moved names the kind, and a record is
 * compared in msg, msgbits, timestampMsg and signalLevel.  The shapes are the ones at which the mask code can go wrong;
 * each checks that it met the boundary it is for.  Prints "avr_rule_units: ok, N", N = the '\n' compared, which the
 * Python test counts again from this file's list. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "msd_avr_impl.h"
#include "msd_wire.h"

#define CHECK(c)                                                                                                        \
    do {                                                                                                              \
        if (!(c)) {                                                                                                   \
            fprintf(stderr, "avr_rule_units: %s:%d: %s (case: %s)\n", __FILE__, __LINE__, #c, what);                  \
            exit(1);                                                                                                  \
        }                                                                                                             \
    } while (0)

static long compared;
static const char *what = "";
static Window W;
static bool rec_ends_at[WIN]; /* a line that yields a record was compared with its '\n' here */

struct Got {
    int n;
    msd_message m;
};

static void on_message(const msd_message *mm, void *user)
{
    Got *g = (Got *)user;
    g->m = *mm;
    ++g->n;
}

static void fill(const std::string &piece, int rmin)
{
    memset(&W, 0, sizeof W);
    for (int r = 0; r < (int)WIN; ++r) {
        const bool in = r >= rmin && r < rmin + (int)piece.size();
        const uint32_t ch = in ? (uint8_t)piece[r - rmin] : 0xffu;
        const uint64_t bit = 1ull << (r & 63);
        W.ch[r] = (uint8_t)ch;
        W.nl[r >> 6] |= is_nl(ch) ? bit : 0;
        W.ws[r >> 6] |= is_ws(ch) ? bit : 0;
        W.nul[r >> 6] |= is_nul(ch) ? bit : 0;
        W.hex[r >> 6] |= is_hex(ch) ? bit : 0;
    }
}

/* What line_at made of the last '\n' of the piece that it was asked about. */
struct Seen {
    int kind, a, skip, plen, r;
};

/* The piece at window position rmin, begun inside an overlong line if `discard`.  Returns the last comparison. */
static Seen run(const std::string &piece, int rmin, int discard, int mode_ac, int keep)
{
    CHECK(rmin >= 0 && rmin + piece.size() <= WIN);
    fill(piece, rmin);
    msd_avr_reader rd;
    msd_avr_reader_init(&rd, mode_ac, keep);
    rd.discard = discard;
    Seen seen = {-1, -1, -1, -1, -1};
    size_t from = 0;
    for (size_t i = 0; i < piece.size(); ++i) {
        if (piece[i] != '\n')
            continue;
        const msd_avr_reader before = rd;
        Got got = {0, {}};
        msd_avr_reader_feed(&rd, (const uint8_t *)piece.data() + from, i + 1 - from, on_message, &got);
        from = i + 1;
        const int moved_long = (int)(rd.long_lines - before.long_lines), moved_drop = (int)(rd.dropped_lines - before.dropped_lines),
                  moved_rec = (int)(rd.frames - before.frames);
        CHECK(rd.lines == before.lines + 1 && moved_long + moved_drop + moved_rec == 1 && got.n == moved_rec);
        const int want = moved_long ? L_LONG : moved_drop ? L_DROP : L_REC;
        const int r = rmin + (int)i;
        if (r < (int)LB) /* no thread owns it in this window */
            continue;
        int a = -1, skip = -1, plen = -1;
        const int kind = line_at(W, r, rmin, discard != 0, mode_ac, a, skip, plen);
        CHECK(kind == want);
        if (kind == L_REC) {
            msd_message o;
            put_record(W, a, skip, plen, keep, o);
            CHECK(memcmp(o.msg, got.m.msg, sizeof o.msg) == 0);
            CHECK(o.msgbits == got.m.msgbits && o.timestampMsg == got.m.timestampMsg);
            CHECK(o.signalLevel == got.m.signalLevel);
            rec_ends_at[r] = true;
        }
        seen = Seen{kind, a, skip, plen, r};
        ++compared;
    }
    return seen;
}

static const std::string P28 = "8D4840D6202CC371C32CE0576098", P14 = "5D4840D6A1B2C3", P4 = "7700";
static const std::string TS = "0123456789AB";

static std::string payload(int digits)
{
    return digits == 28 ? P28 : digits == 14 ? P14 : P4;
}

/* "\n" + text + "\n" with the text's first byte at window position at; every option pair a line can depend on */
static Seen line(const std::string &text, int at, int mode_ac = 1, int keep = 1)
{
    return run("\n" + text + "\n", at - 1, 0, mode_ac, keep);
}

/* a line at a few places: behind the look-back, across a mask-word seam and across a thread seam */
static void lines(const char *name, const std::string &text, int want, int mode_ac = 1, int keep = 1)
{
    what = name;
    const int at[] = {(int)LB + 3, 64 * 7 - 5, 64 * 9 + (int)PER * 2 - 1, (int)WIN - 1 - (int)text.size()};
    for (int p : at)
        CHECK(line(text, p, mode_ac, keep).kind == want);
}

int main()
{
    /* window positions: a short record line ending at every r of the span */
    what = "window positions";
    const std::string shortline = "*" + P14 + ";";
    for (int r = (int)LB; r < (int)WIN; ++r) {
        const Seen s = line(shortline, r - (int)shortline.size());
        CHECK(s.kind == L_REC && s.r == r && s.a == r - (int)shortline.size());
    }
    for (int r = (int)LB; r < (int)WIN; ++r)
        CHECK(rec_ends_at[r]);

    /* payloads across a seam: the first digit at these bit offsets of a mask word; then with a digit that is none at
     * either end, which the all-hex test must see in whichever word it lies */
    what = "payloads across a seam";
    for (int digits : {4, 14, 28})
        for (int off : {0, 1, 36, 37, 63})
            for (const std::string &head : {std::string("*"), "<" + TS + "7F"}) {
                const int first = 64 * 8 + off;
                std::string good = head + payload(digits) + ";", bad0 = good, bad1 = good;
                bad0[head.size()] = 'G';
                bad1[head.size() + digits - 1] = 'g';
                const Seen s = line(good, first - (int)head.size());
                CHECK(s.kind == L_REC && ((s.a + s.skip) & 63) == off && s.plen == digits);
                CHECK(((off + digits > 64) == (((s.a + s.skip + digits - 1) >> 6) != ((s.a + s.skip) >> 6))));
                CHECK(line(bad0, first - (int)head.size()).kind == L_DROP);
                CHECK(line(bad1, first - (int)head.size()).kind == L_DROP);
            }

    /* the guard word: the longest line ending at the window's last byte, its last digits read with the word behind */
    what = "guard word";
    {
        const std::string l = "<" + TS + "7F" + P28 + ";";
        const Seen s = line(l, (int)WIN - 1 - (int)l.size());
        CHECK(s.kind == L_REC && s.r == (int)WIN - 1 && ((s.a + s.skip) >> 6) == (int)NW - 1 && ((s.a + s.skip) & 63) != 0);
    }

    /* line length: MSD_AVR_LINE_MAX bytes in front of the '\n' are a line, one more is an overlong one */
    const std::string rec = ":" + P28 + ";";
    const std::string fits = std::string(MSD_AVR_LINE_MAX - rec.size(), ' ') + rec, over = " " + fits, over2 = "  " + fits;
    what = "line length";
    for (int at : {(int)LB + 1, 64 * 6 + 9}) {
        CHECK(line(fits, at).kind == L_REC);
        CHECK(line(over, at).kind == L_LONG);
    }

    /* The start of the piece: the same with no '\n' in front, so that r - REACH is rmin - 1, rmin and rmin + 1, with the
     * piece's first byte at the start of the span (a stream's first window) and inside the look-back (a group's
     * segment), begun outside and inside an overlong line.  A '\n' that a thread owns is at LB or behind it, so with
     * rmin = 0 more than REACH bytes lie in front of it: there the line is overlong whatever `discard` says. */
    what = "start of the piece";
    for (int rmin : {(int)LB, 77, (int)LB - 1})
        for (int discard : {0, 1}) {
            const std::string *text[3] = {&fits, &over, &over2};
            for (int d = -1; d <= 1; ++d) {
                const Seen s = run(*text[d + 1] + "\n", rmin, discard, 1, 1);
                CHECK(s.r - REACH == rmin + d && s.kind == (d < 0 && !discard ? L_REC : L_LONG));
            }
        }
    for (int discard : {0, 1}) {
        const std::string fill_lb = std::string(LB - rec.size(), ' ') + rec; /* its '\n' at LB, the first a thread owns */
        const Seen s = run(fill_lb + "\n" + rec + "\n", 0, discard, 1, 1);
        CHECK(s.kind == L_REC && s.r == (int)(LB + 1 + rec.size()));
        CHECK(run(fill_lb + "\n", 0, discard, 1, 1).kind == L_LONG);
    }

    /* prefixes: all five, with the payload one digit short, right and one digit long */
    for (const std::string &head : {std::string("*"), std::string(":"), "@" + TS, "%" + TS, "<" + TS + "7F"})
        for (int digits : {14, 28}) {
            const std::string p = payload(digits);
            lines("prefix, one digit short", head + p.substr(1) + ";", L_DROP);
            lines("prefix", head + p + ";", L_REC);
            lines("prefix, one digit long", head + p + "0;", L_DROP);
        }
    lines("unknown prefix", "#" + P14 + ";", L_DROP);
    lines("prefix only", "<" + TS + ";", L_DROP);

    lines("Mode A/C off", "*" + P4 + ";", L_DROP, 0);
    lines("Mode A/C on", "*" + P4 + ";", L_REC, 1);
    lines("missing ;", "*" + P14, L_DROP);

    lines("NUL before", std::string(1, '\0') + "*" + P14 + ";", L_DROP);
    lines("NUL inside", "*" + P14.substr(0, 6) + std::string(1, '\0') + P14.substr(7) + ";", L_DROP);
    lines("NUL after", "*" + P14 + ";" + std::string(1, '\0') + "*" + P28, L_REC);
    lines("NUL last", "*" + P14 + ";" + std::string(1, '\0'), L_REC);
    lines("NUL in front of the ;", "*" + P14 + std::string(1, '\0') + ";", L_DROP);

    lines("white space only", " \t\r\v\f ", L_DROP);
    lines("empty", "", L_DROP);
    lines("\\r\\n", "*" + P28 + ";\r", L_REC);
    lines("tabs", "\t\t@" + TS + P14 + ";\t ", L_REC);

    lines("non-hex first digit", "*" + std::string("x") + P28.substr(1) + ";", L_DROP);
    lines("non-hex last digit", "*" + P28.substr(0, 27) + "/;", L_DROP);
    for (int keep : {0, 1}) {
        lines("non-hex timestamp", "@01234G6789AB" + P14 + ";", L_REC, 1, keep);
        lines("timestamp", "%" + TS + P28 + ";", L_REC, 1, keep);
    }
    for (const char *sig : {"G1", "1G", "GG", " 7", "ff"})
        lines("non-hex signal", "<" + TS + sig + P14 + ";", L_REC);

    printf("avr_rule_units: ok, %ld\n", compared);
    return 0;
}
