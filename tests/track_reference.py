"""numpy float32 reference of the tracking stage, written from its definition (include/fmcw.h,
fmcw_track_params) and not from the kernel: a plain sort of all admissible pairs where the kernel
takes wave minima, Python lists where it uses ballots, one np.float32 rounding per operation in the
order the definition writes them.  The device results are compared with it exactly.

A sequence's state is a dict of per-slot arrays (id, status, hits, misses, age int32; r, v, d, power
float32) and the id counter; pack_state / unpack_state map it to the bytes of the device's state
block (id, status, hits, misses, age, r, v, d, power as max_trk words each, the counter, zero padding
to 16 bytes), which lets the GPU tests compare the final state as well."""
import numpy as np

F32 = np.float32
INT_KEYS = ("trk_id", "trk_status", "trk_age", "trk_misses")
FLOAT_KEYS = ("trk_range", "trk_range_rate", "trk_doppler", "trk_power")
OUT_KEYS = ("trk_count",) + INT_KEYS + FLOAT_KEYS + ("tgt_track",)
IN_KEYS = ("tgt_count", "range", "doppler", "peak_power")
_SLOT_I = ("id", "status", "hits", "misses", "age")
_SLOT_F = ("r", "v", "d", "power")


def state_bytes(max_trk):
    return 4 * ((9 * max_trk + 1 + 3) // 4 * 4)


def fresh_state(max_trk):
    st = {k: np.zeros(max_trk, np.int32) for k in _SLOT_I}
    st.update({k: np.zeros(max_trk, np.float32) for k in _SLOT_F})
    st["counter"] = 0
    return st


def pack_state(st):
    T = len(st["id"])
    w = np.zeros(state_bytes(T) // 4, np.uint32)
    for i, k in enumerate(_SLOT_I):
        w[i * T:(i + 1) * T] = st[k].view(np.uint32)
    for i, k in enumerate(_SLOT_F):
        w[(5 + i) * T:(6 + i) * T] = st[k].view(np.uint32)
    w[9 * T] = st["counter"] & 0xffffffff
    return w.view(np.uint8)


def unpack_state(b, max_trk):
    T = max_trk
    w = np.ascontiguousarray(b, np.uint8).view(np.uint32)
    assert w.size == state_bytes(T) // 4
    st = {k: w[i * T:(i + 1) * T].view(np.int32).copy() for i, k in enumerate(_SLOT_I)}
    st.update({k: w[(5 + i) * T:(6 + i) * T].view(np.float32).copy() for i, k in enumerate(_SLOT_F)})
    st["counter"] = int(w[9 * T])
    return st


def _bits(c):
    return int(np.array(c, np.float32).view(np.uint32))


def _free(st, k):
    for key in _SLOT_I:
        st[key][k] = 0
    for key in _SLOT_F:
        st[key][k] = F32(0)


def frame_step(st, q, nr, nd, count, zr, zd, zp):
    """One frame of one sequence, in place on `st`.  zr, zd, zp: float32 [max_tgt].  Returns the
    frame's outputs (a dict of rows)."""
    T, M = int(q.max_trk), len(zr)
    gr, gd = float(F32(q.gate_r)), float(F32(q.gate_d))
    with np.errstate(all="ignore"):
        wr, wd = F32(1.0 / (gr * gr)), F32(1.0 / (gd * gd))
        ar, ad, br = F32(q.alpha_r), F32(q.alpha_d), F32(q.beta_r)
        n = min(max(int(count), 0), M)
        valid = [j for j in range(n) if np.isfinite(zr[j]) and np.isfinite(zd[j]) and
                 F32(0.5) <= zr[j] < F32(nr + 0.5) and F32(0.5) <= zd[j] < F32(nd + 0.5)]
        # 1. predict
        live = [k for k in range(T) if st["status"][k] != 0]
        rp = {k: F32(st["r"][k] + st["v"][k]) for k in live}
        # 2. cost
        # (float32 arrays: numpy rounds every elementwise operation to float32 on its own)
        pairs, er_of, x_of = [], {}, {}
        if live and valid:
            er = zr[valid][None, :] - np.array([rp[k] for k in live], np.float32)[:, None]
            x = zd[valid][None, :] - st["d"][live][:, None]
            x = np.where(x >= F32(nd // 2), x - F32(nd), np.where(x < F32(-(nd // 2)), x + F32(nd), x))
            c = (er * er) * wr + (x * x) * wd
            assert er.dtype == x.dtype == c.dtype == np.float32
            for a, b in zip(*np.nonzero(c <= F32(1.0))):
                k, j = live[a], valid[b]
                er_of[k, j], x_of[k, j] = er[a, b], x[a, b]
                pairs.append((1 if st["status"][k] == 1 else 0, _bits(c[a, b]), k, j))
        # 3. greedy association over the sorted pairs
        slot_of, meas_of = {}, {}
        for _, _, k, j in sorted(pairs):
            if k not in meas_of and j not in slot_of:
                meas_of[k], slot_of[j] = j, k
        tgt_track = np.zeros(M, np.int32)
        for j, k in slot_of.items():
            tgt_track[j] = st["id"][k]
        # 4. update
        for k in live:
            if k in meas_of:
                j = meas_of[k]
                er, x = er_of[k, j], x_of[k, j]
                if st["hits"][k] == 1:
                    st["r"][k], st["v"][k], st["d"][k] = zr[j], er, zd[j]
                else:
                    st["r"][k] = F32(rp[k] + F32(ar * er))
                    st["v"][k] = F32(st["v"][k] + F32(br * er))
                    dn = F32(st["d"][k] + F32(ad * x))
                    if dn >= F32(nd + 0.5):
                        dn = F32(dn - F32(nd))
                    if dn < F32(0.5):
                        dn = F32(dn + F32(nd))
                    st["d"][k] = dn
                st["power"][k] = zp[j]
                st["hits"][k] += np.int32(1)
                st["misses"][k] = 0
                st["age"][k] += np.int32(1)
                if st["status"][k] == 1 and st["hits"][k] >= q.confirm_hits:
                    st["status"][k] = 2
            else:
                st["r"][k] = rp[k]
                st["misses"][k] += np.int32(1)
                st["age"][k] += np.int32(1)
                if st["status"][k] == 1 or st["misses"][k] > q.max_coast:
                    _free(st, k)
            if st["status"][k] != 0 and not (st["r"][k] >= F32(0.5) and st["r"][k] < F32(nr + 0.5)):
                _free(st, k)
        # 5. births
        free = [k for k in range(T) if st["status"][k] == 0]
        for j in valid:
            if j in slot_of or not free:
                continue
            k = free.pop(0)
            st["counter"] = (st["counter"] + 1) & 0xffffffff
            st["id"][k] = np.uint32(st["counter"]).astype(np.int32)
            st["status"][k] = 2 if q.confirm_hits == 1 else 1
            st["hits"][k], st["misses"][k], st["age"][k] = 1, 0, 1
            st["r"][k], st["v"][k], st["d"][k], st["power"][k] = zr[j], F32(0), zd[j], zp[j]
            tgt_track[j] = st["id"][k]
    # 6. outputs
    return dict(trk_count=np.int32((st["status"] == 2).sum()), trk_id=st["id"].copy(), trk_status=st["status"].copy(),
                trk_age=st["age"].copy(), trk_misses=st["misses"].copy(), trk_range=st["r"].copy(),
                trk_range_rate=st["v"].copy(), trk_doppler=st["d"].copy(), trk_power=st["power"].copy(),
                tgt_track=tgt_track)


def reference_of(tgts, q, nr, nd, n_seq=1, state=None):
    """The outputs of fmcw_track over tgts (tgt_count [S*F]; range, doppler, peak_power
    [S*F][max_tgt]) and the packed final state uint8 [S][state_bytes].  state: packed bytes or None."""
    cnt = np.asarray(tgts["tgt_count"], np.int32)
    zr, zd, zp = (np.asarray(tgts[k], np.float32) for k in ("range", "doppler", "peak_power"))
    rows, M, T = len(cnt), zr.shape[1], int(q.max_trk)
    assert rows % n_seq == 0
    F = rows // n_seq
    out = dict(trk_count=np.zeros(rows, np.int32), tgt_track=np.zeros((rows, M), np.int32))
    for k in INT_KEYS:
        out[k] = np.zeros((rows, T), np.int32)
    for k in FLOAT_KEYS:
        out[k] = np.zeros((rows, T), np.float32)
    packed = np.zeros((n_seq, state_bytes(T)), np.uint8)
    for s in range(n_seq):
        st = fresh_state(T) if state is None else unpack_state(np.asarray(state, np.uint8).reshape(n_seq, -1)[s], T)
        for f in range(F):
            row = s * F + f
            res = frame_step(st, q, nr, nd, cnt[row], zr[row], zd[row], zp[row])
            for k, v in res.items():
                out[k][row] = v
        packed[s] = pack_state(st)
    out["state"] = packed
    return out


def assert_same(got, ref, keys=OUT_KEYS + ("state",)):
    """Exact, bit for bit (NaN payloads and signed zeros included)."""
    for k in keys:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            w = {1: np.uint8, 4: np.uint32}[a.itemsize]
            at = tuple(np.argwhere(a.view(w) != b.view(w))[0])
            raise AssertionError(f"{k}: first difference at {list(at)}: got {a[at]!r}, want {b[at]!r}")
