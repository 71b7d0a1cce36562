// pose_ring.h — the reuse proof of the pose rings (ctx.h: the zero-copy ring, N = 32 pinned slots; the big-pose ring, N = 8 device blocks).
// Pure arithmetic: needs neither HIP nor ctx.h, so a stand-alone program can hold it to a brute-force model (tests/pose_ring_main.cpp).
//
// Upload u takes slot u % N, whose previous tenant is upload u - N. Nothing hands a slot back per frame; instead ONE event is recorded every
// P = N / 2 uploads, on the stream the readers run on, BEFORE the upload it is recorded in front of: the event of sequence s covers every
// reader of the uploads below s. Two events are kept, of alternating multiples of P. The tenant u - N is read by frames launched before upload
// u - N + 1, so the event to poll is that of the first multiple of P that is >= u - N + 1: it is <= u - P — recorded at least half a ring
// ago, normally long signalled — and it is the older of the two events kept.
#pragma once
#include <cstdint>

namespace rzring {

template <int N> struct ReuseProof {
    static_assert(N >= 2 && N % 2 == 0, "two events share the ring");
    static constexpr uint64_t P = N / 2;
    uint64_t uploads = 0;                       // uploads taken so far = the index u of the next one
    uint64_t seq[2] = { ~0ull, ~0ull };         // the sequence each event was last recorded at (~0 = never)

    // the event to record in front of upload u, or -1; recorded(e) once the record has been enqueued
    int record_event() const { return uploads % P == 0 ? (int)((uploads / P) & 1) : -1; }
    void recorded(int e) { seq[e] = uploads; }
    // upload u reuses a slot (false: the ring's first N uploads poll nothing); then the sequence and the event to poll, and whether that
    // event still holds that sequence (false: the bookkeeping is inconsistent — refuse, never poll)
    bool reuses() const { return uploads >= (uint64_t)N; }
    uint64_t poll_seq() const { return (uploads - (N - 1) + (P - 1)) / P * P; }
    int poll_event() const { return (int)((poll_seq() / P) & 1); }
    bool held() const { return seq[poll_event()] == poll_seq(); }
    // the slot of upload u; the next call speaks of upload u + 1
    int take() { return (int)(uploads++ % N); }
};

}  // namespace rzring
