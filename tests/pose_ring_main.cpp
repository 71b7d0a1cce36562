// The reuse proof of the pose rings (reze-engine_amd/csrc/pose_ring.h) against a brute-force model, for the two ring sizes in use: N = 32
// (zero-copy slots) and N = 8 (big-pose blocks). Stand-alone: built with g++ -fsanitize=address,undefined by tests/helpers.py and run by
// tests/test_pose_ring_cpu.py. The model keeps what the proof does not: for every event the sequence it was LAST recorded at, written down
// by this program at the moment it "records", and for every slot the upload that filled it.
#include "../reze-engine_amd/csrc/pose_ring.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond, ...)                                                       \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond);      \
            std::printf(__VA_ARGS__);                                          \
            std::printf("\n");                                                 \
            std::exit(1);                                                      \
        }                                                                      \
    } while (0)

template <int N> static long walk(rzring::ReuseProof<N> &proof, const char *what)
{
    const long long P = N / 2, none = -1;
    long long model_seq[2] = { none, none };        // the sequence each event was last recorded at
    std::vector<long long> tenant(N, none);         // the upload that filled each slot
    long polls = 0;
    for (long long u = 0; u <= 4 * N + 3; ++u) {
        CHECK((long long)proof.uploads == u, "%s N=%d u=%lld", what, N, u);
        // (a) an event is recorded exactly when u % (N / 2) == 0, and the two events alternate
        const int rec = proof.record_event();
        CHECK((rec >= 0) == (u % P == 0), "%s N=%d u=%lld rec=%d", what, N, u, rec);
        if (rec >= 0) {
            CHECK(rec == (int)((u / P) % 2), "%s N=%d u=%lld rec=%d", what, N, u, rec);
            model_seq[rec] = u;
            proof.recorded(rec);
        }
        CHECK(proof.reuses() == (u >= N), "%s N=%d u=%lld", what, N, u);
        if (u >= N) {
            // (b) the event polled covers every reader of the slot's previous tenant — upload u - N, read by frames launched before upload
            // u - N + 1 — and was recorded at least half a ring ago; brute force: it is the first multiple of P that does
            const long long s = (long long)proof.poll_seq();
            CHECK(u - N + 1 <= s && s <= u - P, "%s N=%d u=%lld polls sequence %lld", what, N, u, s);
            long long first = u - N + 1;
            while (first % P) ++first;
            CHECK(s == first, "%s N=%d u=%lld polls %lld, the first covering record is %lld", what, N, u, s, first);
            CHECK(tenant[u % N] == u - N && tenant[u % N] < s, "%s N=%d u=%lld tenant %lld", what, N, u, tenant[u % N]);
            // (c) that record has not been overwritten by a later one, in the model and in the proof's own books
            const int e = proof.poll_event();
            CHECK(e == 0 || e == 1, "%s N=%d u=%lld e=%d", what, N, u, e);
            CHECK(model_seq[e] == s, "%s N=%d u=%lld event %d holds %lld, polled for %lld", what, N, u, e, model_seq[e], s);
            CHECK(proof.held(), "%s N=%d u=%lld", what, N, u);
            ++polls;
        }
        const int slot = proof.take();
        CHECK(slot == (int)(u % N), "%s N=%d u=%lld slot=%d", what, N, u, slot);
        tenant[slot] = u;
    }
    return polls;
}

template <int N> static void ring()
{
    rzring::ReuseProof<N> proof;
    const long polls = walk(proof, "fresh");
    CHECK(polls == 3 * N + 4, "N=%d polls=%ld", N, polls);
    // a re-allocated ring starts over: its first N uploads poll nothing (walk asserts reuses() == (u >= N) from u = 0 again)
    proof = {};
    walk(proof, "after a reset");
    // corrupted books: the event to poll no longer holds the sequence the proof needs -> "inconsistent", at every phase of the period
    for (int k = 0; k < N; ++k) {
        rzring::ReuseProof<N> bad;
        for (int u = 0; u < N + k; ++u) {
            const int rec = bad.record_event();
            if (rec >= 0) bad.recorded(rec);
            bad.take();
        }
        const int rec = bad.record_event();
        if (rec >= 0) bad.recorded(rec);
        CHECK(bad.reuses() && bad.held(), "N=%d k=%d", N, k);
        const unsigned long long kept = bad.seq[bad.poll_event()];
        bad.seq[bad.poll_event()] = kept + N / 2;       // as if a later record had overwritten it
        CHECK(!bad.held(), "N=%d k=%d later record", N, k);
        bad.seq[bad.poll_event()] = ~0ull;              // as if it had never been recorded
        CHECK(!bad.held(), "N=%d k=%d never recorded", N, k);
        bad.seq[bad.poll_event()] = kept;
        bad.uploads += N;                               // an upload count that ran a whole ring ahead of its records
        CHECK(!bad.held(), "N=%d k=%d uploads ahead", N, k);
    }
    std::printf("N=%d ok: %ld polls over %d uploads\n", N, polls, 4 * N + 4);
}

int main()
{
    ring<8>();
    ring<32>();
    return 0;
}
