// What the tool writes, each thing in one place for the one-file path and the batch path: the number formats, the event lines, the
// level table, the rising edges and NumPy files.
#pragma once

#include <algorithm>
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace {

// Swift's description of a Double / Float: the shortest digits that round-trip, with ".0" for whole numbers.
template <typename F>
std::string swift_number(F v)
{
    char buf[64];
    auto r = std::to_chars(buf, buf + sizeof buf, v);
    std::string s(buf, r.ptr);
    if (s.find_first_of(".en") == std::string::npos) s += ".0";   // "2" -> "2.0"; leaves "1e+16", "inf", "nan"
    return s;
}

// The same under Swift 4.0 / 4.1, the toolchain the project declares (SWIFT_VERSION = 4.0, project.pbxproj:593): before
// Swift 4.2 `description` printed "%0.*g" with digits10 significant digits -- 15 for Double, 6 for Float -- and appended ".0" when
// the text held neither '.', 'e' nor a letter.  The one output line the reference holds, in its help text (main.swift:33),
// "0,1593298,36.1292063492063,0.918557", is in this form: 15 and 6 digits.
template <typename F>
std::string swift4_number(F v)
{
    char buf[64];
    std::snprintf(buf, sizeof buf, "%0.*g", sizeof(F) == 8 ? 15 : 6, (double)v);
    std::string s(buf);
    if (s.find_first_of(".eEn") == std::string::npos) s += ".0";          // ("inf", "nan" keep their letters)
    return s;
}

bool g_swift4 = false;                                     // --format swift4
template <typename F>
std::string number(F v) { return g_swift4 ? swift4_number(v) : swift_number(v); }

// the rc of a run over many files from the status r of one path: device trouble (2) is fatal for the exit code; an unreadable
// file (1) is skipped, and a product that could not be written (3: the lines are out, the file is not) costs 1
void fold_status(int &rc, int r)
{
    if (r == 2) rc = 2;
    else if (r == 3 && rc == 0) rc = 1;
}

// one event line: channel,sample,seconds,out0[,out1...]
std::string event_line(const std::string &channel, int64_t sample, double rate, const float *values, int n_out)
{
    std::string line = channel + "," + std::to_string(sample) + "," + number((double)sample / rate);
    for (int o = 0; o < n_out; o++) line += "," + number(values[o]);
    return line;
}

// One track's events as a path found them: the samples, and event i's outputs at value + (index ? index[i] : i) * n_out
struct TrackEvents {
    const int64_t *sample;
    const int64_t *index;
    int64_t n;
    const float *value;
};

// The lines of one file: the tracks' events interleaved buffer by buffer, --chunk frames a buffer (0: channel by channel)
void print_events(const std::vector<TrackEvents> &tracks, int n_out, int64_t chunk, double rate)
{
    struct Event { int64_t buffer; int channel; int64_t sample; const float *value; };
    std::vector<Event> events;
    for (size_t c = 0; c < tracks.size(); c++)
        for (int64_t i = 0; i < tracks[c].n; i++) {
            const int64_t smp = tracks[c].sample[i];
            events.push_back({chunk > 0 ? (smp - 1) / chunk : 0, (int)c, smp, tracks[c].value + (size_t)(tracks[c].index ? tracks[c].index[i] : i) * n_out});
        }
    // the reference's loop hands every track one buffer per round (main.swift:126-130)
    std::stable_sort(events.begin(), events.end(), [](const Event &a, const Event &b) {
        if (a.buffer != b.buffer) return a.buffer < b.buffer;
        if (a.channel != b.channel) return a.channel < b.channel;
        return a.sample < b.sample;
    });
    for (const Event &ev : events) std::puts(event_line(std::to_string(ev.channel), ev.sample, rate, ev.value, n_out).c_str());
    std::fflush(stdout);
}

// --format-line: formats one event line from its parts (channel sample rate out0 [out1 ...]; the outputs as fp32) exactly as the
// event loop does: the known-answer test of the number formats, no audio and no GPU involved
void format_line(int n, char **parts)
{
    std::vector<float> values;
    for (int k = 3; k < n; k++) values.push_back(std::strtof(parts[k], nullptr));
    std::puts(event_line(parts[0], std::atoll(parts[1]), std::strtod(parts[2], nullptr), values.data(), (int)values.size()).c_str());
}

// The level meters of one file: its tracks' readings in three tables, track c's from first[c]
struct LevelTable {
    int tracks, buffer;                                     // ... and the samples of a buffer
    int64_t P, M, fed;                                      // buffers a reading, readings, samples the detector was fed
    const int64_t *first;
    const double *in;                                       // mean squares
    const float *out;
    const uint8_t *empty;                                   // the reading holds no evaluation
};

// ... written reading by reading, track by track: track, time of the reading's end, input RMS, output level (empty: no evaluation)
bool write_levels(const std::string &path, const LevelTable &t, double rate)
{
    FILE *f = std::fopen(path.c_str(), "w");
    bool ok = f != nullptr;
    const int64_t PL = std::min(t.P, (t.fed + t.buffer - 1) / t.buffer) * t.buffer;
    for (int64_t m = 0; ok && m < t.M; m++)
        for (int c = 0; ok && c < t.tracks; c++) {
            const size_t at = (size_t)(t.first[c] + m);
            const std::string line = std::to_string(c) + "\t" + number((double)std::min((m + 1) * PL, t.fed) / rate) + "\t" +
                                     number(std::sqrt(t.in[at])) + "\t" + (t.empty[at] ? std::string() : number(t.out[at])) + "\n";
            ok = std::fputs(line.c_str(), f) >= 0;
        }
    if (f && std::fclose(f) != 0) ok = false;
    if (!ok) std::fprintf(stderr, "Unable to write %s.\n", path.c_str());
    return ok;
}

// the rising edges as --ttl-onsets writes them: track, sample, seconds
bool write_onsets(const std::string &path, int C, const int64_t *idx, const int64_t *cnt, int64_t cap, double rate)
{
    FILE *f = std::fopen(path.c_str(), "w");
    bool ok = f != nullptr;
    for (int c = 0; ok && c < C; c++)
        for (int64_t i = 0; ok && i < std::min(cnt[(size_t)c], cap); i++) {
            const int64_t smp = idx[(size_t)c * (size_t)cap + (size_t)i];
            const std::string line = std::to_string(c) + "\t" + std::to_string(smp) + "\t" + number((double)smp / rate) + "\n";
            ok = std::fputs(line.c_str(), f) >= 0;
        }
    if (f && std::fclose(f) != 0) ok = false;
    if (!ok) std::fprintf(stderr, "Unable to write %s.\n", path.c_str());
    return ok;
}

// NumPy format 1.0, little endian, C order
bool write_npy(const std::string &path, const char *descr, const std::vector<int64_t> &shape, const void *data, size_t bytes)
{
    std::string dict = std::string("{'descr': '") + descr + "', 'fortran_order': False, 'shape': (";
    for (size_t i = 0; i < shape.size(); i++) dict += std::to_string(shape[i]) + (shape.size() == 1 || i + 1 < shape.size() ? "," : "") + (i + 1 < shape.size() ? " " : "");
    dict += "), }";
    while ((10 + dict.size() + 1) % 64 != 0) dict += ' ';
    dict += '\n';
    FILE *f = std::fopen(path.c_str(), "wb");
    bool ok = f != nullptr;
    const unsigned char head[10] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0, (unsigned char)(dict.size() & 255), (unsigned char)(dict.size() >> 8)};
    ok = ok && std::fwrite(head, 1, 10, f) == 10 && std::fwrite(dict.data(), 1, dict.size(), f) == dict.size() && (bytes == 0 || std::fwrite(data, 1, bytes, f) == bytes);
    if (f && std::fclose(f) != 0) ok = false;
    if (!ok) std::fprintf(stderr, "Unable to write %s.\n", path.c_str());
    return ok;
}

}  // namespace
