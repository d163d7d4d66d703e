// multi_gpu.hip — see multi_gpu.hpp.  Host code (one thread per GPU) + one small kernel; the exchanges are RCCL calls.
#include "multi_gpu.hpp"

#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>
#include <thread>

namespace edsx {

// ---------------------------------------------------------------------------------------------------------------
// exchanges
// ---------------------------------------------------------------------------------------------------------------
void Exchange::all_gather_v(int rank, int world, const void* mine, size_t bytes, std::vector<uint8_t>& all, std::vector<u64>& sizes)
{
    sizes.assign(world, 0);
    const u64 my = bytes;
    all_gather(rank, &my, sizeof(my), sizes.data());
    u64 cap = 1;
    for (u64 s : sizes) cap = std::max(cap, s);
    std::vector<uint8_t> pad(cap, 0);
    if (bytes) std::memcpy(pad.data(), mine, bytes);
    all.resize((size_t)cap * world);
    all_gather(rank, pad.data(), cap, all.data());
}

namespace {

class LocalExchange final : public Exchange {           // rank threads of one process, any device assignment
public:
    explicit LocalExchange(int n) : n_(n), bar_(n) {}
    void all_gather(int rank, const void* mine, size_t bytes, void* all) override
    {
        { std::lock_guard<std::mutex> g(mu_); if (stage_.size() < (size_t)n_ * bytes) stage_.resize((size_t)n_ * bytes); }
        bar_.arrive(rank, nullptr);                      // the staging area has its size
        std::memcpy(stage_.data() + (size_t)rank * bytes, mine, bytes);
        bar_.arrive(rank, nullptr);                      // every contribution is in
        std::memcpy(all, stage_.data(), (size_t)n_ * bytes);
        bar_.arrive(rank, nullptr);                      // everyone has read it: the area may be reused
    }
    const char* name() const override { return "in-process"; }
private:
    int n_; RankBarrier bar_; std::mutex mu_; std::vector<uint8_t> stage_;
};

#define EDSX_NCCL(call)                                                                       \
    do {                                                                                      \
        ncclResult_t r__ = (call);                                                            \
        if (r__ != ncclSuccess) throw DeviceError(std::string(#call) + ": " + ncclGetErrorString(r__)); \
    } while (0)

class RcclExchange final : public Exchange {            // one communicator, stream and pair of staging buffers per rank
public:
    explicit RcclExchange(const std::vector<int>& devices) : dev_(devices), comm_(devices.size()), st_(devices.size()),
                                                              send_(devices.size()), recv_(devices.size())
    {
        EDSX_NCCL(ncclCommInitAll(comm_.data(), (int)dev_.size(), dev_.data()));
        for (size_t r = 0; r < dev_.size(); r++) {
            EDSX_HIP(hipSetDevice(dev_[r]));
            EDSX_HIP(hipStreamCreateWithFlags(&st_[r], hipStreamNonBlocking));
        }
    }
    ~RcclExchange() override
    {
        for (size_t r = 0; r < dev_.size(); r++) {
            (void)hipSetDevice(dev_[r]);
            (void)hipStreamDestroy(st_[r]);
            (void)ncclCommDestroy(comm_[r]);
            send_[r].release(); recv_[r].release();
        }
    }
    void all_gather(int rank, const void* mine, size_t bytes, void* all) override
    {
        const size_t n = dev_.size();
        send_[rank].ensure(bytes + 16); recv_[rank].ensure(n * bytes + 16);
        EDSX_HIP(hipMemcpyAsync(send_[rank].ptr, mine, bytes, hipMemcpyHostToDevice, st_[rank]));
        EDSX_NCCL(ncclAllGather(send_[rank].ptr, recv_[rank].ptr, bytes, ncclUint8, comm_[rank], st_[rank]));
        EDSX_HIP(hipMemcpyAsync(all, recv_[rank].ptr, n * bytes, hipMemcpyDeviceToHost, st_[rank]));
        EDSX_HIP(hipStreamSynchronize(st_[rank]));
    }
    const char* name() const override { return "rccl"; }
private:
    std::vector<int> dev_; std::vector<ncclComm_t> comm_; std::vector<hipStream_t> st_;
    std::vector<DevBuf> send_, recv_;
};

// header of every row of a row image: ">r", blanks, newline; and the newline behind the row's columns
__global__ void k_row_frames(uint8_t* __restrict__ img, u64 nrows, u64 ncols, u64 h0, u64 h)
{
    const u64 wave = (blockIdx.x * (u64)blockDim.x + threadIdx.x) >> 6, nwaves = ((u64)gridDim.x * blockDim.x) >> 6;
    const u32 lane = threadIdx.x & 63;
    for (u64 r = wave; r < nrows; r += nwaves) {
        const u64 hl = r ? h : h0;
        uint8_t* p = img + (r ? h0 + (ncols + 1) + (r - 1) * (h + ncols + 1) : 0);
        for (u64 i = lane; i < hl; i += 64) p[i] = i == 0 ? '>' : i == 1 ? 'r' : i + 1 == hl ? '\n' : ' ';
        if (lane == 0) p[hl + ncols] = '\n';
    }
}

} // namespace

// ---------------------------------------------------------------------------------------------------------------
// Row image: columns [c0, c1) of every row of a host FASTA image as a one-line-per-row image in HBM whose rows all begin
// on multiples of 128 bytes (blank-padded headers).  The column scan reads every row in 128-byte pieces; from a
// 128-byte-aligned row those loads are aligned, and the scan of the 1000 x 100 Mb alignment takes 21.8 instead of
// 26.9 ms (round 3, bench.py "aligned_rows").  A row's slab is one contiguous piece of the file (one-line rows), so
// the upload is a 2D copy per stretch of equally spaced rows; wrapped rows are put together on the host.
// ---------------------------------------------------------------------------------------------------------------
RowImage upload_row_image(const uint8_t* fasta, const MsaLayout& lay, u64 c0, u64 c1, DevBuf& d_img, std::vector<uint8_t>& host_tmp,
                          hipStream_t st)
{
    RowImage ri;
    const u64 S = lay.start.size(), ncols = c1 - c0;
    ri.rows = S; ri.cols = ncols;
    ri.hdr0 = 128;
    ri.hdr = (128 - (ncols + 1) % 128) % 128;
    if (ri.hdr < 8) ri.hdr += 128;
    ri.bytes = ri.hdr0 + S * (ncols + 1) + (S - 1) * ri.hdr;
    d_img.ensure(ri.bytes + 16);
    uint8_t* img = d_img.as<uint8_t>();
    const u64 pitch = ri.hdr + ncols + 1;                      // rows 1 .. S-1
    auto data_off = [&](u64 r) { return r ? ri.hdr0 + (ncols + 1) + (r - 1) * pitch + ri.hdr : ri.hdr0; };
    if (lay.lw == 0) {
        // rows with headers of equal length are equally spaced in the file: one 2D copy per such stretch of rows
        EDSX_HIP(hipMemcpyAsync(img + data_off(0), fasta + lay.start[0] + c0, ncols, hipMemcpyHostToDevice, st));
        for (u64 s0 = 1; s0 < S;) {
            u64 s1 = s0;                                       // last row of the stretch
            const u64 sp = s0 + 1 < S ? lay.start[s0 + 1] - lay.start[s0] : pitch;
            while (s1 + 1 < S && lay.start[s1 + 1] - lay.start[s1] == sp) s1++;
            const u64 nrows = s1 - s0 + 1;
            EDSX_HIP(hipMemcpy2DAsync(img + data_off(s0), pitch, fasta + lay.start[s0] + c0, sp, ncols, nrows, hipMemcpyHostToDevice, st));
            s0 += nrows;
        }
    } else {
        // wrapped rows: columns [c0, c1) of a row are the bytes c + c / lw without the newlines between them
        host_tmp.resize(S * ncols);
        for (u64 s = 0; s < S; s++) row_columns(fasta, lay, s, c0, c1, host_tmp.data() + s * ncols);
        EDSX_HIP(hipMemcpyAsync(img + data_off(0), host_tmp.data(), ncols, hipMemcpyHostToDevice, st));
        if (S > 1) EDSX_HIP(hipMemcpy2DAsync(img + data_off(1), pitch, host_tmp.data() + ncols, ncols, ncols, S - 1, hipMemcpyHostToDevice, st));
    }
    hipLaunchKernelGGL(k_row_frames, dim3(64), dim3(256), 0, st, img, S, ncols, ri.hdr0, ri.hdr);
    EDSX_HIP(hipGetLastError());
    return ri;
}

// an alignment image of n bytes in d_img on the current device -> plan, emit, download
void msa_image_to_text(MsaPipeline& p, const DevBuf& d_img, size_t n, uint32_t l, DevBuf& d_eds, DevBuf& d_seds, HostBytes& eds,
                       HostBytes& seds, hipStream_t st)
{
    uint64_t E = 0, Q = 0;
    p.plan(d_img.as<uint8_t>(), n, l, st, &E, &Q);
    d_eds.ensure(E);
    d_seds.ensure(Q);
    p.emit(d_eds.as<uint8_t>(), d_seds.as<uint8_t>(), st);
    eds.take(E);
    seds.take(Q);
    PinnedDownload::copy(eds.data, d_eds.ptr, E, st);
    PinnedDownload::copy(seds.data, d_seds.ptr, Q, st);
}

void msa_transform_plain(MsaPipeline& p, const uint8_t* msa, size_t n, uint32_t l, DevBuf& d_img, DevBuf& d_eds, DevBuf& d_seds,
                         HostBytes& eds, HostBytes& seds, hipStream_t st)
{
    d_img.ensure(n);
    EDSX_HIP(hipMemcpyAsync(d_img.ptr, msa, n, hipMemcpyHostToDevice, st));
    msa_image_to_text(p, d_img, n, l, d_eds, d_seds, eds, seds, st);
}

// ---------------------------------------------------------------------------------------------------------------
// MultiMsa
// ---------------------------------------------------------------------------------------------------------------
MultiMsa::MultiMsa(const std::vector<int>& devices, bool use_rccl) : devices_(devices)
{
    if (devices.empty()) throw ParamError("edsx_multi_create: no devices");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) throw DeviceError("no usable gfx950 device (the engine has no CPU fallback)");
    for (int d : devices) if (d < 0 || d >= count) throw ParamError("edsx_multi_create: device id out of range");
    if (use_rccl) {
        std::vector<int> sorted = devices;
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            throw ParamError("edsx_multi_create: RCCL needs one distinct device per rank (use the in-process exchange to share a device)");
        xch_.reset(new RcclExchange(devices));
    } else xch_.reset(new LocalExchange((int)devices.size()));
    bar_.reset(new RankBarrier((int)devices.size()));
    for (int d : devices) { ranks_.emplace_back(new Rank()); ranks_.back()->device = d; }
}

MultiMsa::~MultiMsa()
{
    for (auto& r : ranks_) { (void)hipSetDevice(r->device); r.reset(); }
}

void MultiMsa::transform(const uint8_t* fasta, size_t n, uint32_t context_len, HostBytes& eds, HostBytes& seds)
{
    const int N = world();
    if (n == 0) throw FormatError("Invalid MSA: empty input");
    MsaLayout lay;
    if (N > 1) lay = msa_layout(fasta, n);
    partitioned_ = slabs_fit(lay, N, context_len);
    chains_ = 0;
    auto whole_on_rank0 = [&] {
        // One GPU: a file that is not a plain uniform alignment gets its error from the transform itself, in the reference's
        // words; an l-EDS whose slabs have no standalone common run to anchor the stitch on is not partitioned either.
        Rank& r0 = *ranks_[0];
        EDSX_HIP(hipSetDevice(r0.device));
        msa_transform_plain(r0.slab, fasta, n, context_len, r0.d_img, r0.d_eds, r0.d_seds, eds, seds, nullptr);
    };
    if (!partitioned_) { whole_on_rank0(); return; }
    no_anchor_ = false;
    // (no typed rethrow here: a failed rank's text decides between a format error and a device error)
    try {
        run_ranks([&](int r) { run_rank(r, fasta, lay, context_len, eds, seds); }, nullptr);
    } catch (const DeviceError& ex) {
        if (std::string(ex.what()).rfind("Invalid MSA", 0) == 0) throw FormatError(ex.what());
        throw;
    }
    if (no_anchor_) { partitioned_ = false; chains_ = 0; whole_on_rank0(); }
}

// The rank threads of one call: ranks 1 .. N-1 on threads of their own, rank 0 on the caller's.  After a failure (the
// barrier keeps the one of the lowest rank) that rank's own exception is thrown again where the caller has kept them
// (`errors`, one per rank), else a DeviceError with its text.
void MultiMsa::run_ranks(const std::function<void(int)>& one_rank, const std::vector<std::exception_ptr>* errors)
{
    const int N = world();
    bar_->reset();
    std::vector<std::thread> th;
    for (int r = 1; r < N; r++) th.emplace_back([&, r] { one_rank(r); });
    one_rank(0);
    for (auto& t : th) t.join();
    if (!bar_->failed()) return;
    const int fr = bar_->failed_rank();
    if (errors && fr >= 0 && fr < N && (*errors)[fr]) std::rethrow_exception((*errors)[fr]);
    throw DeviceError(bar_->message());
}

// ---------------------------------------------------------------------------------------------------------------
// The two device steps of a slab transform, for the ranks and for the column batches alike
// ---------------------------------------------------------------------------------------------------------------
namespace {

// columns [c0, c1) as a row image -> HBM, plan, emit: E and Q bytes of text in d_eds / d_seds, and the slab pipeline
// answers edge_info / anchor_info
void describe_slab(const SlabWorker& w, const uint8_t* fasta, const MsaLayout& lay, u64 c0, u64 c1, uint32_t l, hipStream_t st,
                   uint64_t& E, uint64_t& Q)
{
    const RowImage ri = upload_row_image(fasta, lay, c0, c1, *w.d_img, *w.host, st);
    w.slab->plan(w.d_img->as<uint8_t>(), ri.bytes, l, st, &E, &Q);
    w.d_eds->ensure(E); w.d_seds->ensure(Q);
    w.slab->emit(w.d_eds->as<uint8_t>(), w.d_seds->as<uint8_t>(), st);
}

// a boundary's mini alignment through the second pipeline; its text is appended to extra_e / extra_s
void recompute_boundary(const SlabWorker& w, const std::vector<uint8_t>& mini, uint32_t l, hipStream_t st, std::vector<uint8_t>& extra_e,
                        std::vector<uint8_t>& extra_s)
{
    w.d_mini->ensure(mini.size() + 16);
    EDSX_HIP(hipMemcpyAsync(w.d_mini->ptr, mini.data(), mini.size(), hipMemcpyHostToDevice, st));
    uint64_t e2 = 0, q2 = 0;
    w.mini->plan(w.d_mini->as<uint8_t>(), mini.size(), l, st, &e2, &q2);
    DevBuf oe, oq;
    oe.ensure(e2); oq.ensure(q2);
    w.mini->emit(oe.as<uint8_t>(), oq.as<uint8_t>(), st);
    const size_t pe = extra_e.size(), pq = extra_s.size();
    extra_e.resize(pe + e2); extra_s.resize(pq + q2);
    EDSX_HIP(hipMemcpyAsync(extra_e.data() + pe, oe.ptr, e2, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipMemcpyAsync(extra_s.data() + pq, oq.ptr, q2, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
}

} // namespace

// One rank, either context length (the stitch itself: msa_slabs.hpp).  Every phase ends in the thread barrier, which also
// carries a failure of any rank to all of them: nobody enters a collective that a failed rank will not join.
void MultiMsa::run_rank(int r, const uint8_t* fasta, const MsaLayout& lay, uint32_t l, HostBytes& eds, HostBytes& seds)
{
    const int N = world();
    Rank& me = *ranks_[r];
    const SlabWorker w = me.worker();
    std::string fail;
    auto phase = [&](auto&& body) -> bool { return rank_phase(*bar_, r, fail, body); };    // false: some rank failed, leave
    const u64 S = lay.start.size(), c0 = slab_cut(lay.L, r, N), c1 = slab_cut(lay.L, r + 1, N);
    hipStream_t st = nullptr;
    uint64_t E = 0, Q = 0;
    SlabEdges my_edges{};
    SlabAnchors my_anchors{};
    std::vector<SlabEdges> edges(l ? 0 : N);
    std::vector<SlabAnchors> anchors(l ? N : 0);

    // ---- 1. slab image -> HBM, plan, emit, the descriptor: edges (l = 0) or anchors
    if (!phase([&] {
            EDSX_HIP(hipSetDevice(me.device));
            describe_slab(w, fasta, lay, c0, c1, l, st, E, Q);
            if (l) my_anchors = slab_anchors(w.slab->anchor_info(l, st), r, N, c1 - c0, E, Q);
            else my_edges = slab_edges(w.slab->edge_info(st), c1 - c0, E, Q);
        })) return;

    // ---- 2. all-gather of the descriptors (twelve u64 either way); the same stitch on every rank
    if (!phase([&] {
            if (l) xch_->all_gather(r, &my_anchors, sizeof(SlabAnchors), anchors.data());
            else xch_->all_gather(r, &my_edges, sizeof(SlabEdges), edges.data());
        })) return;
    bool ok = true;
    const SlabStitch stitch = l ? stitch_from_anchors(anchors, ok) : stitch_from_edges(edges);
    if (!ok) { if (r == 0) no_anchor_ = true; return; }                 // the same on every rank
    if (r == 0) chains_ = stitch.chains;
    const SlabKeep keep = stitch.keep[r];

    // ---- 3. only when a boundary is recomputed (l = 0: a variant run crosses a cut; l > 0: always): all-gather of the
    // raw columns of every job's parts (padded to the largest contribution: every rank derives all block sizes from the
    // descriptors), the owners recompute their segments
    std::vector<uint8_t> extra_e, extra_s;
    if (!stitch.jobs.empty()) {
        const u64 cap = std::max<u64>(1, S * stitch.max_cols);
        std::vector<uint8_t> buf(cap, 0), all((size_t)cap * N);
        if (!phase([&] {
                EDSX_HIP(hipSetDevice(me.device));
                for (const SlabJob& j : stitch.jobs)
                    for (const SlabPart& p : j.parts)
                        if (p.slab == r) w.slab->copy_columns(p.col0, p.ncols, buf.data() + S * p.before, st);
            })) return;
        if (!phase([&] { xch_->all_gather(r, buf.data(), cap, all.data()); })) return;
        if (!phase([&] {
                EDSX_HIP(hipSetDevice(me.device));
                std::vector<std::pair<const uint8_t*, u64>> blocks;           // row-major blocks of the same rows
                for (const SlabJob& j : stitch.jobs) {
                    if (j.owner != r) continue;
                    blocks.clear();
                    for (const SlabPart& p : j.parts) blocks.emplace_back(all.data() + (size_t)p.slab * cap + S * p.before, p.ncols);
                    mini_image(S, blocks, *w.host);
                    recompute_boundary(w, *w.host, l, st, extra_e, extra_s);
                }
            })) return;
    }

    // ---- 4. piece sizes (an all-gather only when some segment was recomputed), offsets, the output buffers
    std::vector<u64> sizes(2 * (size_t)N);
    if (!stitch.jobs.empty()) {
        const u64 my[2] = {(keep.ehi - keep.elo) + extra_e.size(), (keep.shi - keep.slo) + extra_s.size()};
        if (!phase([&] { xch_->all_gather(r, my, sizeof(my), sizes.data()); })) return;
    } else
        for (int rk = 0; rk < N; rk++) {
            sizes[2 * rk] = stitch.keep[rk].ehi - stitch.keep[rk].elo;
            sizes[2 * rk + 1] = stitch.keep[rk].shi - stitch.keep[rk].slo;
        }
    u64 eoff, soff, etot, stot;
    piece_offsets(sizes, 2, r, eoff, soff, etot, stot);
    if (!phase([&] { if (r == 0) { eds.take(etot); seds.take(stot); } })) return;

    // ---- 5. every rank writes its piece at its offset
    phase([&] {
        EDSX_HIP(hipSetDevice(me.device));
        if (keep.ehi > keep.elo) PinnedDownload::copy(eds.data + eoff, w.d_eds->as<uint8_t>() + keep.elo, keep.ehi - keep.elo, st);
        if (keep.shi > keep.slo) PinnedDownload::copy(seds.data + soff, w.d_seds->as<uint8_t>() + keep.slo, keep.shi - keep.slo, st);
        if (!extra_e.empty()) std::memcpy(eds.data + eoff + (keep.ehi - keep.elo), extra_e.data(), extra_e.size());
        if (!extra_s.empty()) std::memcpy(seds.data + soff + (keep.shi - keep.slo), extra_s.data(), extra_s.size());
    });
}

// ---------------------------------------------------------------------------------------------------------------
// Column batches on ONE GPU (edsx_msa_transform_batched, and what edsx_msa_transform falls back to when an alignment and
// its tables do not fit the device): the slabs of the multi-GPU path one after the other through one pipeline.  The
// working set is that of one slab (image, variant columns, records, tables); every slab's text goes to the host as soon
// as it is written, the boundaries are stitched at the end exactly as between ranks - but the boundary columns come
// straight from the host image, and the pieces are put together with host copies.
// ---------------------------------------------------------------------------------------------------------------
bool msa_transform_batched(const SlabWorker& w, const uint8_t* fasta, const MsaLayout& lay, uint32_t l, int K,
                           HostBytes& eds, HostBytes& seds, hipStream_t st)
{
    if (!slabs_fit(lay, K, l)) return false;
    const u64 S = lay.start.size();
    std::vector<HostBytes> pe(K), ps(K);
    std::vector<SlabEdges> edges(l ? 0 : K);
    std::vector<SlabAnchors> anchors(l ? K : 0);

    // ---- 1. every slab: image -> HBM, plan, emit, descriptor, text -> host
    for (int r = 0; r < K; r++) {
        const u64 c0 = slab_cut(lay.L, r, K), c1 = slab_cut(lay.L, r + 1, K);
        uint64_t E = 0, Q = 0;
        describe_slab(w, fasta, lay, c0, c1, l, st, E, Q);
        if (l) {
            anchors[r] = slab_anchors(w.slab->anchor_info(l, st), r, K, c1 - c0, E, Q);
            if (!anchors[r].ok) return false;                 // no anchors: not batched
        } else edges[r] = slab_edges(w.slab->edge_info(st), c1 - c0, E, Q);
        pe[r].take(E); ps[r].take(Q);
        PinnedDownload::copy(pe[r].data, w.d_eds->ptr, E, st);
        PinnedDownload::copy(ps[r].data, w.d_seds->ptr, Q, st);
    }

    // ---- 2. boundaries: which bytes of every slab's text stay, and the text recomputed behind them.  The parts of a job
    // are neighbours in the alignment: one block of the host image from the first part's first column to behind the last's
    bool ok = true;
    const SlabStitch stitch = l ? stitch_from_anchors(anchors, ok) : stitch_from_edges(edges);
    std::vector<std::vector<uint8_t>> xe(K), xs(K);
    std::vector<uint8_t> block, mini;
    for (const SlabJob& j : stitch.jobs) {
        const SlabPart &a = j.parts.front(), &b = j.parts.back();
        const u64 g0 = slab_cut(lay.L, a.slab, K) + a.col0, g1 = slab_cut(lay.L, b.slab, K) + b.col0 + b.ncols;
        block.resize(S * (g1 - g0));
        for (u64 s = 0; s < S; s++) row_columns(fasta, lay, s, g0, g1, block.data() + s * (g1 - g0));
        mini_image(S, {{block.data(), g1 - g0}}, mini);
        recompute_boundary(w, mini, l, st, xe[j.owner], xs[j.owner]);
    }

    // ---- 3. the pieces in order
    u64 etot = 0, stot = 0;
    for (int r = 0; r < K; r++) {
        const SlabKeep& k = stitch.keep[r];
        etot += (k.ehi - k.elo) + xe[r].size(); stot += (k.shi - k.slo) + xs[r].size();
    }
    eds.take(etot); seds.take(stot);
    u64 eo = 0, so = 0;
    for (int r = 0; r < K; r++) {
        const SlabKeep& k = stitch.keep[r];
        std::memcpy(eds.data + eo, pe[r].data + k.elo, k.ehi - k.elo); eo += k.ehi - k.elo;
        std::memcpy(seds.data + so, ps[r].data + k.slo, k.shi - k.slo); so += k.shi - k.slo;
        if (!xe[r].empty()) { std::memcpy(eds.data + eo, xe[r].data(), xe[r].size()); eo += xe[r].size(); }
        if (!xs[r].empty()) { std::memcpy(seds.data + so, xs[r].data(), xs[r].size()); so += xs[r].size(); }
    }
    return true;
}

} // namespace edsx
