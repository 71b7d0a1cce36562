"""VMD IK on / off keys and the per-chain switches of the IK stage, restated in NumPy beside ik_ref.py: the definition the device
(rz_set_ik_enabled / rz_upload_ik_keys, kernels/ik.hip.h: ik_stage<SW>), the host solver (host/model.js: Model.solveIK with
setIKChainEnabled) and the sampler (host/vmd-sampler.js: ikStateAt) are held to.

A motion's show / IK block is a list of keys, each a frame and a list of (chain name, enabled). flatten() turns it into a step function
per chain: key_frame[n], non-descending, and key_enabled[n][n_chains]. state_at() evaluates it; choose() picks the clip of a cross-fade
state whose switches apply; solve() is ik_ref.solve over the chains that are on. Switch states are pure comparisons: the same in every
precision, matched exactly."""
import numpy as np

import ik_ref

NO_CLIP = 0xffffffff


def flatten(keys, chain_names):
    """keys = [dict(frame, ik=[dict(name, enabled)])] (the loader's ikFrames) or [(frame, [(name, enabled)])]; chain_names = the model's
    chains in table order. Keys are stably sorted by frame; a chain a key does not name keeps its state from the key before it; a chain is
    enabled before any key has named it; names the model lacks are ignored. Returns (key_frame [n] float32, key_enabled [n][n_chains] uint8)."""
    norm = []
    for k in keys:
        if isinstance(k, dict):
            norm.append((float(k["frame"]), [(e["name"], bool(e["enabled"])) for e in k["ik"]]))
        else:
            norm.append((float(k[0]), [(n, bool(e)) for n, e in k[1]]))
    order = sorted(range(len(norm)), key=lambda i: norm[i][0])          # (sorted is stable)
    index = {n: i for i, n in enumerate(chain_names)}
    state = np.ones(len(chain_names), dtype=np.uint8)
    kf = np.zeros(len(norm), dtype=np.float32)
    ke = np.ones((len(norm), len(chain_names)), dtype=np.uint8)
    for r, i in enumerate(order):
        for name, en in norm[i][1]:
            if name in index:
                state[index[name]] = 1 if en else 0
        kf[r] = norm[i][0]
        ke[r] = state
    return kf, ke


def state_at(key_frame, key_enabled, frame, n_chains=None):
    """The row of the LAST key with key_frame <= frame, compared as float32 values (among keys on equal frames the last one wins); for a
    frame before the first key the first key's row; with no keys all chains are on."""
    kf = np.asarray(key_frame, dtype=np.float32).reshape(-1)
    if kf.size == 0:
        n = n_chains if n_chains is not None else np.asarray(key_enabled).shape[-1]
        return np.ones(n, dtype=np.uint8)
    ke = np.asarray(key_enabled, dtype=np.uint8).reshape(kf.size, -1)
    f = np.float32(frame)
    last = -1
    for k in range(kf.size):
        if kf[k] <= f:
            last = k
    return ke[max(last, 0)].copy()


def choose(state, key_sets, n_chains):
    """state = (clip_a, frame_a, clip_b, frame_b, blend); key_sets = {clip: (key_frame, key_enabled)}. Clip A's row at frame_a applies when
    clip_b == NO_CLIP or blend < 0.5 (as float32), otherwise clip B's row at frame_b; a chosen clip without keys gives all on. Layers never
    switch IK."""
    clip_a, frame_a, clip_b, frame_b, blend = state
    use_b = int(clip_b) != NO_CLIP and not (np.float32(blend) < np.float32(0.5))
    clip, frame = (int(clip_b), frame_b) if use_b else (int(clip_a), frame_a)
    if clip not in key_sets or key_sets[clip] is None:
        return np.ones(n_chains, dtype=np.uint8)
    return state_at(key_sets[clip][0], key_sets[clip][1], frame, n_chains)


def solve(parents, bind, q, t=None, chains=(), enabled=None, **kw):
    """ik_ref.solve over the chains whose switch is on (enabled[k] goes with chains[k]; None = all on), in the same order. A chain that is
    off does nothing: its links keep the rotations of `q`, as a chain with loops == 0 does."""
    chains = list(chains)
    if enabled is not None:
        en = np.asarray(enabled).reshape(-1)
        assert en.size == len(chains), (en.size, len(chains))
        chains = [ch for ch, e in zip(chains, en) if e]
    return ik_ref.solve(parents, bind, q, t, chains, **kw)
