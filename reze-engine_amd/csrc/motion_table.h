// motion_table.h — the host half of rz_upload_animation and rz_upload_motions that needs no GPU: what the two calls check of a flattened
// motion (rz_animation, include/reze_deform.h) and the arrays they upload. One flattener serves both: the keys of all clips concatenated,
// the records carrying absolute indices — a library of one clip is the single motion's arrays, base 0. Plain C++ without HIP, beside
// after_table.h: tests/motion_table_main.cpp compiles it alone, and tests/test_motion_table_cpu.py holds what it prints to the
// concatenation restated in numpy. Keys of tracks that drive nothing of this model (a bone it lacks, a morph track no feed names) are never
// read by a kernel and are not looked at.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/reze_deform.h"

#pragma GCC visibility push(hidden)
namespace rzmotion {

// neither NaN nor infinite: the one finite check of the motion stack (keys here; frames, blends and weights in pose.cpp)
inline bool finite(float x) { return x == x && x - x == 0.0f; }

// What is checked of one motion, and what is derived from it: bone_track[b] = the track that drives bone b or -1, feed_off[M + 1] = the
// feeds of the model's vertex morphs (all zero without morph tracks; feed_off[M] = their count). False with the refusal in `err`.
inline bool check(uint32_t B, uint32_t M, const rz_animation *a, std::vector<int> &bone_track, std::vector<uint32_t> &feed_off, std::string &err)
{
    auto no = [&err](const std::string &why) { err = why; return false; };
    auto key_no = [&no](const char *track, uint32_t t, uint32_t k, const char *what) { return no(std::string(track) + " " + std::to_string(t) + " key " + std::to_string(k) + ": the " + what + " is not finite"); };
    if (!a) return no("null animation");
    if (B == 0) return no("upload the skeleton before a motion");
    const uint32_t n = a->n_bone_tracks, mt = a->n_morph_tracks;
    if (n && (!a->track_bone || !a->key_off || !a->key_frame || !a->key_rot4 || !a->key_pos3)) return no("null bone-track arrays");
    if (mt && (!a->mkey_off || !a->mkey_frame || !a->mkey_weight)) return no("null morph-track arrays");
    if (M && mt && (!a->feed_off || (a->feed_off[M] && (!a->feed_track || !a->feed_ratio)))) return no("null morph feeds");
    bone_track.assign(B, -1);
    for (uint32_t t = 0; t < n; ++t) {
        if (a->key_off[t] > a->key_off[t + 1]) return no("key offsets must be non-decreasing");
        const int32_t b = a->track_bone[t];
        if (b < 0 || (uint32_t)b >= B) continue;                         // a motion may key bones this model lacks
        if (bone_track[b] >= 0) return no("bone " + std::to_string(b) + " is driven by two tracks");
        for (uint32_t k = a->key_off[t] + 1; k < a->key_off[t + 1]; ++k)
            // equal frames are legal (real VMD files carry duplicate keys; host/vmd-sampler.js keeps them too): the span search
            // lands on the last key <= frame and the first key > frame, so a zero-length span is never divided by
            if (!(a->key_frame[k] >= a->key_frame[k - 1])) return no("track " + std::to_string(t) + ": key frames must not descend");
        // every key of a track that drives a bone of this model is finite: a NaN frame passes no comparison of the span search, an
        // infinite one makes the guessed span's index undefined, and either in a rotation or a position is a NaN pose nothing explains
        for (uint32_t k = a->key_off[t]; k < a->key_off[t + 1]; ++k) {
            if (!finite(a->key_frame[k])) return key_no("track", t, k - a->key_off[t], "frame");
            for (int d = 0; d < 4; ++d)
                if (!finite(a->key_rot4[(size_t)k * 4 + d])) return key_no("track", t, k - a->key_off[t], "rotation");
            for (int d = 0; d < 3; ++d)
                if (!finite(a->key_pos3[(size_t)k * 3 + d])) return key_no("track", t, k - a->key_off[t], "position");
        }
        bone_track[b] = (int)t;
    }
    for (uint32_t t = 0; t < mt; ++t) {
        if (a->mkey_off[t] > a->mkey_off[t + 1]) return no("morph key offsets must be non-decreasing");
        for (uint32_t k = a->mkey_off[t] + 1; k < a->mkey_off[t + 1]; ++k)
            if (!(a->mkey_frame[k] >= a->mkey_frame[k - 1])) return no("morph track " + std::to_string(t) + ": key frames must not descend");
    }
    feed_off.assign(M + 1, 0);
    if (M && mt) {
        for (uint32_t m = 0; m <= M; ++m) feed_off[m] = a->feed_off[m];
        const uint32_t F = feed_off[M];
        for (uint32_t m = 0; m < M; ++m)
            if (feed_off[m] > feed_off[m + 1]) return no("feed offsets must be non-decreasing");
        for (uint32_t f = 0; f < F; ++f)
            if (a->feed_track[f] < 0 || (uint32_t)a->feed_track[f] >= mt) return no("feed " + std::to_string(f) + " names morph track " + std::to_string(a->feed_track[f]) + " of " + std::to_string(mt));
        // ... and so is every key of a morph track that feeds a vertex morph of this model
        std::vector<char> seen(mt, 0);
        for (uint32_t f = 0; f < F; ++f) {
            const uint32_t t = (uint32_t)a->feed_track[f];
            if (seen[t]) continue;
            seen[t] = 1;
            for (uint32_t k = a->mkey_off[t]; k < a->mkey_off[t + 1]; ++k) {
                if (!finite(a->mkey_frame[k])) return key_no("morph track", t, k - a->mkey_off[t], "frame");
                if (!finite(a->mkey_weight[k])) return key_no("morph track", t, k - a->mkey_off[t], "weight");
            }
        }
    }
    return true;
}

// What is uploaded. A record is four 32-bit words: (first key, one past the last key, bits(first key's frame), bits(last key's frame)) of
// a track, key indices absolute in the concatenated arrays; four zeros for a bone no track drives, a track without keys, and such feeds.
struct Flat {
    std::vector<uint32_t> bone_rec;     // [n_clips][B][4] the track of each bone in each clip
    std::vector<uint32_t> feed_off;     // [n_clips][M + 1] per clip and vertex morph: its feeds, absolute
    std::vector<uint32_t> feed_range;   // [F][4] the morph track of each feed
    std::vector<float> feed_ratio;      // [F]
    std::vector<float> key_frame, key_rot, key_pos;     // [K], [K][4], [K][3]
    std::vector<uint8_t> key_interp;    // [K][16], or empty: no clip with bone tracks carries interpolation bytes
    std::vector<float> mkey_frame, mkey_weight;         // [Km]
};

constexpr uint64_t kIndexLimit = 0xfffffff0ull;         // keys, morph keys and feeds are addressed with 32 bits

// The arrays of `n_clips` motions behind each other. A clip is checked before it is appended; on a refusal `out` is half filled and not to
// be used (the callers replace nothing before flatten() has returned true). `library` = the call's name when the clips are a library:
// it goes in front of the refusals, with the clip's number in front of a clip's own ("rz_upload_motions: clip 2: bone 7 is driven by
// two tracks"); null for the single motion, whose refusals stand bare.
inline bool flatten(uint32_t B, uint32_t M, uint32_t n_clips, const rz_animation *clips, const char *library, Flat &out, std::string &err,
                    uint64_t index_limit = kIndexLimit)
{
    out = Flat();
    bool any_interp = false;
    for (uint32_t k = 0; clips && k < n_clips; ++k) any_interp = any_interp || (clips[k].key_interp16 != nullptr && clips[k].n_bone_tracks != 0);
    // a clip without interpolation bytes beside one that has them: the default curve 20 20 107 107, which bezier_y answers with x itself
    static const uint8_t linear[16] = { 20, 20, 20, 20, 20, 20, 20, 20, 107, 107, 107, 107, 107, 107, 107, 107 };
    auto record = [](std::vector<uint32_t> &to, const uint32_t *off, const float *kf, int t, uint32_t base) {
        uint32_t r[4] = { 0u, 0u, 0u, 0u };
        if (t >= 0 && off[t + 1] != off[t]) {
            r[0] = base + off[t]; r[1] = base + off[t + 1];
            memcpy(&r[2], &kf[off[t]], 4);
            memcpy(&r[3], &kf[off[t + 1] - 1], 4);
        }
        to.insert(to.end(), r, r + 4);
    };
    // (an empty clip hands null arrays over: nothing is appended from a null pointer)
    auto append = [](std::vector<float> &to, const float *from, size_t n) { if (n) to.insert(to.end(), from, from + n); };
    for (uint32_t k = 0; k < n_clips; ++k) {
        const rz_animation *a = clips ? &clips[k] : nullptr;
        std::vector<int> bone_track;
        std::vector<uint32_t> feed_off;
        if (!check(B, M, a, bone_track, feed_off, err)) {
            if (library) err = std::string(library) + ": clip " + std::to_string(k) + ": " + err;
            return false;
        }
        const uint32_t n = a->n_bone_tracks, mt = a->n_morph_tracks, F = feed_off[M];
        const uint32_t K = n ? a->key_off[n] : 0, Km = mt ? a->mkey_off[mt] : 0;
        const size_t key_base = out.key_frame.size(), mkey_base = out.mkey_frame.size(), feed_base = out.feed_ratio.size();
        if (key_base + K > index_limit || mkey_base + Km > index_limit || feed_base + F > index_limit)
            return err = (library ? std::string(library) + ": " : std::string()) + "the library's keys do not fit 32-bit indices", false;
        for (uint32_t b = 0; b < B; ++b) record(out.bone_rec, a->key_off, a->key_frame, bone_track[b], (uint32_t)key_base);
        for (uint32_t m = 0; m <= M; ++m) out.feed_off.push_back((uint32_t)feed_base + feed_off[m]);
        for (uint32_t f = 0; f < F; ++f) {
            record(out.feed_range, a->mkey_off, a->mkey_frame, a->feed_track[f], (uint32_t)mkey_base);
            out.feed_ratio.push_back(a->feed_ratio[f]);
        }
        append(out.key_frame, a->key_frame, K);
        append(out.key_rot, a->key_rot4, (size_t)K * 4);
        append(out.key_pos, a->key_pos3, (size_t)K * 3);
        if (any_interp)
            for (uint32_t j = 0; j < K; ++j) {
                const uint8_t *src = a->key_interp16 ? a->key_interp16 + (size_t)j * 16 : linear;
                out.key_interp.insert(out.key_interp.end(), src, src + 16);
            }
        append(out.mkey_frame, a->mkey_frame, Km);
        append(out.mkey_weight, a->mkey_weight, Km);
    }
    return true;
}

}  // namespace rzmotion
#pragma GCC visibility pop
