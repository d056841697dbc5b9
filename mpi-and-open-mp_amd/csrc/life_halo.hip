// life_halo.hip -- the halo exchange of the device runtime (life_exchange,
// life_cart.c:225-279): phase x (columns), then phase y (rows of width+2),
// each either a periodic fill inside the shard (dims[d] == 1) or grouped
// ncclSend / ncclRecv with the Cartesian neighbours (RCCL transport) or
// device-to-device copies between the shards of this process (LOCAL
// transport).  The plan (life::halo_plan) changes only at creation and at
// LIFE_OPT_LOOPBACK: plan_halos resolves staging slots, copies and wait lists
// there, so that a halo phase between two kernel launches only walks tables.
#include "life_dev_internal.h"

namespace life {
namespace rt {
namespace {

// Pointer + size of the message of op `o` (the slot-th send or recv of its
// kind among its phase's ops of the same `what`): column ops go through the
// staging slots, corner ops (the fused plan) through the corner slots behind
// them, row ops are whole padded rows sent straight from / received straight
// into the buffer (every shard of one Cartesian column has the same pitch).
void op_buffer(const Shard &s, const life_halo_op &o, int slot, uint8_t *base, uint8_t **ptr, size_t *bytes) {
    const size_t cbr = (size_t)life::column_bytes_per_row(s.lay);
    uint8_t *st = o.kind == LIFE_HALO_SEND ? s.col_send : s.col_recv;
    if (o.what == LIFE_HALO_COLUMN) {
        const size_t per = (size_t)s.lay.h * cbr;
        *ptr = st + (size_t)slot * per;
        *bytes = per;
    } else if (o.what == LIFE_HALO_CORNER) {
        const size_t per = (size_t)s.lay.yapron * cbr;
        *ptr = st + 2 * (size_t)s.lay.h * cbr + (size_t)slot * per;
        *bytes = per;
    } else {
        *ptr = base + o.index * s.lay.pitch;
        *bytes = (size_t)(o.width * s.lay.pitch);
    }
}

// The LOCAL transport's copies and wait lists of shard `s` (every shard's
// plan and slots are set): the matching is life::halo_match_send's.
int resolve_local(life_dev *d, Shard &s) {
    auto local_index = [&](int rank) -> int {
        Shard *t = find_local(d, rank);
        if (!t) set_err("LOCAL transport: peer %d not in this process", rank);
        return t ? (int)(t - d->shards.data()) : -1;
    };
    const int n = (int)s.plan.size();
    s.copies.clear();
    for (int i = 0; i < n; i++) {
        const life_halo_op &o = s.plan[i];
        if (o.kind != LIFE_HALO_RECV) continue;
        const int src = local_index(o.peer);
        if (src < 0) return LIFE_ESTATE;
        const Shard &from = d->shards[src];
        // matching send: the kth send from src to s.rank
        const int k = life::halo_match_send(s.plan.data(), i, s.rank, from.plan.data(), (int)from.plan.size());
        if (k < 0) {
            set_err("LOCAL transport: no matching send %d->%d", o.peer, s.rank);
            return LIFE_ESTATE;
        }
        uint8_t *p;
        size_t dn, sn;
        op_buffer(s, o, s.slot[i], s.buf[0], &p, &dn);
        op_buffer(from, from.plan[k], from.slot[k], from.buf[0], &p, &sn);
        if (dn != sn) {
            set_err("LOCAL transport: size mismatch %zu vs %zu", dn, sn);
            return LIFE_ESTATE;
        }
        s.copies.push_back(LocalCopy{o.phase, src, k, from.slot[k], i, s.slot[i], dn});
    }
    for (int phase = 0; phase < 2; phase++)
        for (int kind : {LIFE_HALO_SEND, LIFE_HALO_RECV}) {
            int peers[16];
            const int np = life::halo_wait_peers(s.plan.data(), n, s.rank, phase, kind, peers);
            std::vector<int> &w = s.waits[phase][kind];
            w.clear();
            for (int k = 0; k < np; k++) {
                w.push_back(local_index(peers[k]));
                if (w.back() < 0) return LIFE_ESTATE;
            }
        }
    return LIFE_OK;
}

// LOCAL transport ordering around the copies of one halo phase, peers only
// (an all-to-all barrier cost 8 x 7 stream waits per step of an 8-shard
// pass: 1-2 ms of host time per pass, profiles/r04/b).  kind RECV (before the
// copies): each shard's stream waits for the shards it receives from -- their
// pack / previous phase is queued before their event.  kind SEND (after):
// each shard waits for the shards that copy from it, so nothing it enqueues
// next overwrites a message still being read.
int local_order(life_dev *d, bool comm, int phase, int kind) {
    auto st = [&](Shard &s) { return comm ? s.comm_stream : s.stream; };
    for (Shard &s : d->shards) {
        HIPCHK(hipSetDevice(s.device));
        HIPCHK(hipEventRecord(s.ev_sync, st(s)));
    }
    for (Shard &s : d->shards) {
        HIPCHK(hipSetDevice(s.device));
        for (int t : s.waits[phase][kind]) HIPCHK(hipStreamWaitEvent(st(s), d->shards[t].ev_sync, 0));
    }
    return LIFE_OK;
}

// One halo phase on buffer `which` of every local shard, on stream sel.
int run_phase(life_dev *d, int phase, int which_rel, bool on_comm) {
    auto stream_of = [&](Shard &s) { return on_comm ? s.comm_stream : s.stream; };
    auto buf_of = [&](Shard &s) { return s.buf[s.cur ^ which_rel]; };
    // An axis that is not partitioned (dims[d] == 1, no loopback) has no halo: the stencil
    // wraps it itself (life_kernels.hip, row_ptr / WRAPX), or, for a temporal
    // layout whose width is not a multiple of 32, the shard copies its own
    // edge columns into its x-apron.
    if (!part(d, phase)) {
        if (phase == 0 && self_wrap_x(d))
            for (Shard &s : d->shards) {
                HIPCHK(hipSetDevice(s.device));
                HIPCHK(life::launch_wrap_columns(s.lay, buf_of(s), stream_of(s)));
            }
        return LIFE_OK;
    }
    bool any = false;  // a fused plan (both axes in phase 0) leaves phase 1 empty
    for (const life_halo_op &o : d->shards[0].plan) any |= o.phase == phase;
    if (!any) return LIFE_OK;
    if (phase == 0)
        for (Shard &s : d->shards) {
            HIPCHK(hipSetDevice(s.device));
            HIPCHK(life::launch_pack_columns(s.lay, buf_of(s), s.col_send, stream_of(s), s.corners));
        }
    if (d->transport == LIFE_XPORT_RCCL) {
        NCCLCHK(ncclGroupStart());
        for (Shard &s : d->shards) {
            for (size_t i = 0; i < s.plan.size(); i++) {
                const life_halo_op &o = s.plan[i];
                if (o.phase != phase) continue;
                uint8_t *p;
                size_t nb;
                op_buffer(s, o, s.slot[i], buf_of(s), &p, &nb);
                if (o.kind == LIFE_HALO_SEND)
                    NCCLCHK(ncclSend(p, nb, ncclUint8, o.peer, s.comm, stream_of(s)));
                else
                    NCCLCHK(ncclRecv(p, nb, ncclUint8, o.peer, s.comm, stream_of(s)));
            }
        }
        NCCLCHK(ncclGroupEnd());
    } else {
        CHK(local_order(d, on_comm, phase, LIFE_HALO_RECV));
        for (Shard &s : d->shards) {
            HIPCHK(hipSetDevice(s.device));
            for (const LocalCopy &c : s.copies) {
                if (c.phase != phase) continue;
                Shard &src = d->shards[c.src];
                uint8_t *dp, *sp;
                size_t nb;
                op_buffer(s, s.plan[c.dop], c.dslot, buf_of(s), &dp, &nb);
                op_buffer(src, src.plan[c.sop], c.sslot, buf_of(src), &sp, &nb);
                if (src.device == s.device)
                    HIPCHK(hipMemcpyAsync(dp, sp, c.bytes, hipMemcpyDeviceToDevice, stream_of(s)));
                else
                    HIPCHK(hipMemcpyPeerAsync(dp, s.device, sp, src.device, c.bytes, stream_of(s)));
            }
        }
        CHK(local_order(d, on_comm, phase, LIFE_HALO_SEND));
    }
    if (phase == 0)
        for (Shard &s : d->shards) {
            HIPCHK(hipSetDevice(s.device));
            HIPCHK(life::launch_unpack_columns(s.lay, buf_of(s), s.col_recv, stream_of(s), s.corners));
        }
    return LIFE_OK;
}

}  // namespace

int plan_halos(life_dev *d) {
    for (Shard &s : d->shards) {
        life_halo_op ops[16];
        const int n = life::halo_plan(d->nx, d->ny, d->dims[0], d->dims[1], s.rank, d->kernel, d->loop, ops, 16);
        if (n < 0) {
            set_err("halo plan failed for shard %d", s.rank);
            return LIFE_EINVAL;
        }
        s.plan.assign(ops, ops + n);
        s.corners = std::any_of(s.plan.begin(), s.plan.end(), [](const life_halo_op &o) { return o.what == LIFE_HALO_CORNER; });
        s.slot.clear();
        for (int i = 0; i < n; i++) s.slot.push_back(life::halo_op_slot(ops, i));
    }
    if (d->transport == LIFE_XPORT_LOCAL)
        for (Shard &s : d->shards) CHK(resolve_local(d, s));
    return LIFE_OK;
}

int exchange(life_dev *d, int which_rel, bool on_comm) {
    CHK(run_phase(d, 0, which_rel, on_comm));
    CHK(run_phase(d, 1, which_rel, on_comm));
    d->since = 0;
    return LIFE_OK;
}

}  // namespace rt
}  // namespace life
