// A stand-alone program around reze-engine_amd/csrc/motion_table.h (the GPU-free half of rz_upload_animation and rz_upload_motions): it
// reads motions as text and prints what the call would refuse or upload, for tests/test_motion_table_cpu.py to compare with the
// concatenation restated in numpy. Also the program to build under -fsanitize=address,undefined: every array is allocated at exactly
// the size the motion states, so a read past one is reported. Floats travel as their 32 bits in decimal, both ways (NaN and infinity
// included).
//   input:  library (0 = the single motion: bare refusals, 1 = rz_upload_motions), B, M, n_clips, index limit (0 = the default); per clip:
//             null (bit k set = pointer k of rz_animation is handed over as NULL, in the struct's order; bit 5, the interpolation bytes,
//             is has_interp's to say), has_interp,
//             n_bone_tracks, track_bone[n], key_off[n + 1], then key_frame[K], key_rot4[K][4], key_pos3[K][3], key_interp16[K][16] if has_interp,
//             n_morph_tracks, mkey_off[mt + 1], mkey_frame[Km], mkey_weight[Km], n_feed_off, feed_off[n_feed_off], F, feed_track[F], feed_ratio[F]
//   output: "error <message>", or one line per array of rzmotion::Flat: its name, then its values
#include "../reze-engine_amd/csrc/motion_table.h"

#include <cstdio>
#include <iostream>

namespace {

struct Clip {
    std::vector<int32_t> track_bone, feed_track;
    std::vector<uint32_t> key_off, mkey_off, feed_off;
    std::vector<float> key_frame, key_rot4, key_pos3, mkey_frame, mkey_weight, feed_ratio;
    std::vector<uint8_t> key_interp16;
};

template <class T> void read(std::vector<T> &v, size_t n)
{
    v.resize(n);
    for (T &x : v) { int64_t t; std::cin >> t; x = (T)t; }
    v.shrink_to_fit();
}
void read_bits(std::vector<float> &v, size_t n)
{
    std::vector<uint32_t> b;
    read(b, n);
    v.resize(n);
    if (n) memcpy(v.data(), b.data(), n * 4);
    v.shrink_to_fit();
}
template <class T> const T *ptr(const std::vector<T> &v, bool null) { return null ? nullptr : v.data(); }

void print(const char *name, const std::vector<uint32_t> &v) { printf("%s", name); for (uint32_t x : v) printf(" %u", x); printf("\n"); }
void print(const char *name, const std::vector<uint8_t> &v) { printf("%s", name); for (uint8_t x : v) printf(" %u", x); printf("\n"); }
void print(const char *name, const std::vector<float> &v)
{
    printf("%s", name);
    for (float x : v) { uint32_t b; memcpy(&b, &x, 4); printf(" %u", b); }
    printf("\n");
}

}  // namespace

int main()
{
    uint32_t library, B, M, n_clips;
    uint64_t limit;
    std::cin >> library >> B >> M >> n_clips >> limit;
    if (!std::cin || n_clips == 0 || n_clips > 64 || B > (1u << 20) || M > (1u << 20)) { std::cerr << "bad counts\n"; return 2; }
    std::vector<Clip> data(n_clips);
    std::vector<rz_animation> clips(n_clips);
    for (uint32_t k = 0; k < n_clips; ++k) {
        Clip &c = data[k];
        rz_animation &a = clips[k];
        uint32_t null, has_interp, n, mt, nfo, F;
        std::cin >> null >> has_interp >> n;
        if (!std::cin || n > (1u << 20)) { std::cerr << "short input\n"; return 2; }
        read(c.track_bone, n);
        read(c.key_off, (size_t)n + 1);
        const size_t K = c.key_off[n];
        if (!std::cin || K > (1u << 20)) { std::cerr << "short input\n"; return 2; }
        read_bits(c.key_frame, K);
        read_bits(c.key_rot4, K * 4);
        read_bits(c.key_pos3, K * 3);
        if (has_interp) read(c.key_interp16, K * 16);
        std::cin >> mt;
        if (!std::cin || mt > (1u << 20)) { std::cerr << "short input\n"; return 2; }
        read(c.mkey_off, (size_t)mt + 1);
        const size_t Km = c.mkey_off[mt];
        if (!std::cin || Km > (1u << 20)) { std::cerr << "short input\n"; return 2; }
        read_bits(c.mkey_frame, Km);
        read_bits(c.mkey_weight, Km);
        std::cin >> nfo;
        if (!std::cin || nfo > (1u << 20)) { std::cerr << "short input\n"; return 2; }
        read(c.feed_off, nfo);
        std::cin >> F;
        if (!std::cin || F > (1u << 20)) { std::cerr << "short input\n"; return 2; }
        read(c.feed_track, F);
        read_bits(c.feed_ratio, F);
        if (!std::cin) { std::cerr << "short input\n"; return 2; }
        a.n_bone_tracks = n;
        a.track_bone = ptr(c.track_bone, null & 1u);
        a.key_off = ptr(c.key_off, null & 2u);
        a.key_frame = ptr(c.key_frame, null & 4u);
        a.key_rot4 = ptr(c.key_rot4, null & 8u);
        a.key_pos3 = ptr(c.key_pos3, null & 16u);
        a.key_interp16 = has_interp ? c.key_interp16.data() : nullptr;
        a.n_morph_tracks = mt;
        a.mkey_off = ptr(c.mkey_off, null & 64u);
        a.mkey_frame = ptr(c.mkey_frame, null & 128u);
        a.mkey_weight = ptr(c.mkey_weight, null & 256u);
        a.feed_off = ptr(c.feed_off, (null & 512u) || nfo == 0);
        a.feed_track = ptr(c.feed_track, null & 1024u);
        a.feed_ratio = ptr(c.feed_ratio, null & 2048u);
    }
    rzmotion::Flat f;
    std::string err;
    const bool ok = limit ? rzmotion::flatten(B, M, n_clips, clips.data(), library ? "rz_upload_motions" : nullptr, f, err, limit)
                          : rzmotion::flatten(B, M, n_clips, clips.data(), library ? "rz_upload_motions" : nullptr, f, err);
    if (!ok) { printf("error %s\n", err.c_str()); return 0; }
    print("bone_rec", f.bone_rec);
    print("feed_off", f.feed_off);
    print("feed_range", f.feed_range);
    print("feed_ratio", f.feed_ratio);
    print("key_frame", f.key_frame);
    print("key_rot", f.key_rot);
    print("key_pos", f.key_pos);
    print("key_interp", f.key_interp);
    print("mkey_frame", f.mkey_frame);
    print("mkey_weight", f.mkey_weight);
    return 0;
}
