// capi.hip — the extern "C" boundary declared in include/edsx.h.  No exceptions cross it.
//
// Every convention of the boundary has one definition, in the anonymous namespace below ("The boundary's
// contract"):
//   status_of          exception in flight -> status code and text; guarded(ctx, f) and guarded(multi, f) run f under it
//   clear, zero        out-parameters before anything can fail: buffers {NULL, 0}, structs all zero
//   give, take_copy    an edsx_buf receives a download buffer itself, or a malloc'ed copy of host data
//   put                VcfCounters -> edsx_vcf_stats, with or without variant_groups
//   or_empty           a NULL input of size 0 reads as an empty text
//   vcf_result         the VCF transforms: counters out on success and on failure, then the l-EDS merge, then the buffers
//   in_session         the one-shot entry points: open a session, run on it, close it, keep the status
#include "../../include/edsx.h"

#include "bgzf_device.hpp"
#include "genrandom.hpp"
#include "genvcf.hpp"
#include "gfa_device.hpp"
#include "locate_device.hpp"
#include "merge_device.hpp"
#include "merge_scan.hpp"
#include "msa_device.hpp"
#include "multi_gpu.hpp"
#include "path_device.hpp"
#include "query_device.hpp"
#include "slice_core.hpp"
#include "subset_device.hpp"
#include "synth.hpp"
#include "vcf_contig.hpp"
#include "vcf_device.hpp"
#include "vcf_export_device.hpp"

#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

using namespace edsx;

struct edsx_ctx {
    int device = 0;
    std::string err;
    MsaPipeline msa;
    DeviceEds eds;                           // the tokenised .eds (+ .seds) of the last merge / stats / query / locate call
    MergePipeline merge;
    DevBuf stats_acc;                        // edsx_eds_stats
    RangeScanner scan;                       // edsx_eds_scan_range / edsx_seds_scan_range
    QueryPipeline query;                     // edsx_eds_genpatterns / edsx_eds_check_positions
    LocatePipeline locate;                   // edsx_eds_locate, over query's tables
    SubsetPipeline subset;                   // edsx_eds_subset
    GfaPipeline gfa;                         // edsx_eds_gfa_graph
    VcfExportPipeline vcf_export;            // edsx_eds_vcf
    KernelTimes slice_times;                 // edsx_paths_slice, of every session of this context
    KernelTimes dist_times;                  // edsx_paths_distances, likewise
    KernelTimes ld_times;                    // edsx_paths_ld, likewise
    KernelTimes ibs_times;                   // edsx_paths_ibs, likewise
    KernelTimes mosaic_times;                // edsx_paths_mosaic, likewise
    KernelTimes div_times;                   // edsx_paths_diversity, likewise
    VcfPipeline vcf;
    GenPipeline gen;
    GenVcfPipeline genvcf;
    DevBuf d_in, d_eds, d_seds, synth_desc;
    std::vector<uint8_t> host_tmp;
    std::unique_ptr<MsaPipeline> mini;       // column batches: the boundary segments are recomputed through a second pipeline
    DevBuf d_mini;
    int last_batches = 0;                    // of the last edsx_msa_transform / _batched: 1 = one piece
    GzInfo gz[2];                            // compressed layer of the last *_z / edsx_gz_inflate call: VCF (or input), FASTA
};

struct edsx_multi_impl { std::unique_ptr<MultiMsa> m; std::string err; };

namespace {

// inside a catch (...): the status of the exception in flight, its text into err
int status_of(std::string& err)
{
    try { throw; }
    catch (const FormatError& ex) { err = ex.what(); return EDSX_ERR_INVALID_FORMAT; }
    catch (const ParamError& ex) { err = ex.what(); return EDSX_ERR_INVALID_PARAMETER; }
    catch (const LimitError& ex) { err = ex.what(); return EDSX_ERR_BUILD_FAILED; }
    catch (const DeviceError& ex) { err = ex.what(); return EDSX_ERR_BUILD_FAILED; }
    catch (const std::bad_alloc&) { err = "out of host memory"; return EDSX_ERR_BUILD_FAILED; }
    catch (const std::exception& ex) { err = ex.what(); return EDSX_ERR_UNKNOWN; }
}

template <class F> int guarded(edsx_ctx* ctx, F&& f)
{
    if (!ctx) return EDSX_ERR_INVALID_PARAMETER;
    try {
        ctx->err.clear();
        hipError_t e = hipSetDevice(ctx->device);
        if (e != hipSuccess) throw DeviceError(std::string("hipSetDevice: ") + hipGetErrorString(e));
        f();
        return EDSX_OK;
    } catch (...) { return status_of(ctx->err); }
}

// the multi handle: its ranks choose their devices themselves
template <class F> int guarded(edsx_multi_impl* mi, F&& f)
{
    if (!mi) return EDSX_ERR_INVALID_PARAMETER;
    try {
        mi->err.clear();
        f();
        return EDSX_OK;
    } catch (...) { return status_of(mi->err); }
}

template <class... B> void clear(B*... bufs)
{
    for (edsx_buf* b : {static_cast<edsx_buf*>(bufs)...}) if (b) { b->data = nullptr; b->size = 0; }
}

template <class T> void zero(T* out) { if (out) std::memset(out, 0, sizeof(*out)); }

// the download buffer itself
void give(edsx_buf* b, HostBytes& h)
{
    b->size = h.size;
    b->data = h.release();
}

void take_copy(edsx_buf* b, const void* src, size_t n)
{
    b->data = HostBytes::alloc(n);
    b->size = n;
    if (n) std::memcpy(b->data, src, n);
}

void put(edsx_vcf_stats* stats, const VcfCounters& c, bool groups)
{
    if (!stats) return;
    stats->total_variants = c.total_variants; stats->processed_variants = c.processed_variants;
    stats->skipped_malformed = c.skipped_malformed; stats->skipped_unsupported_sv = c.skipped_unsupported_sv;
    if (groups) stats->variant_groups = c.variant_groups;
}

const uint8_t* or_empty(const uint8_t* p)
{
    static const uint8_t none = 0;
    return p ? p : &none;
}

// run(e, s, c) is a VCF transform.  The reference counts while parsing, before it can throw: the counters of the parse
// survive a later error (variant_groups is known only after the transform).  context_len > 0: merge(e, s) turns the EDS
// text into the l-EDS - LINEAR merge with defaults (compact), vcf_transforms.cpp:735-755 - with the counters already out.
template <class Run, class Merge>
void vcf_result(Run&& run, Merge&& merge, uint32_t context_len, edsx_buf* eds, edsx_buf* seds, edsx_vcf_stats* stats)
{
    HostBytes e, s;
    VcfCounters c;
    try { run(e, s, c); } catch (...) { put(stats, c, false); throw; }
    put(stats, c, true);
    if (context_len > 0) merge(e, s);
    give(eds, e);
    give(seds, s);
}

void merge_in_place(edsx_ctx* ctx, HostBytes& e, HostBytes& s, uint32_t context_len)
{
    HostBytes lo, so;
    ctx->merge.run(ctx->eds, e.data, e.size, s.data, s.size, context_len, true, lo, so, nullptr);
    std::swap(e.data, lo.data); std::swap(e.size, lo.size);
    std::swap(s.data, so.data); std::swap(s.size, so.size);
}

// `opened` is the status of opening the session s: run body on it and close it.  The body's status is the call's, and
// ctx->err stays: closing reports nothing.
template <class S, class Body> int in_session(int opened, S*& s, void (*close)(S*), Body&& body)
{
    if (opened != EDSX_OK) return opened;
    const int rc = body();
    close(s);
    return rc;
}

// everything the MSA entry points hold on the device goes back to the allocator
void release_msa_buffers(edsx_ctx* ctx)
{
    ctx->d_in.release(); ctx->d_eds.release(); ctx->d_seds.release(); ctx->d_mini.release();
    ctx->msa.~MsaPipeline();
    new (&ctx->msa) MsaPipeline();
    ctx->mini.reset();
}

// one piece: upload, plan, emit, download
void msa_transform_whole(edsx_ctx* ctx, const uint8_t* msa, size_t msa_size, const MsaLayout& lay, uint32_t context_len,
                         edsx_buf* eds, edsx_buf* seds)
{
    hipStream_t st = nullptr;
    // A plain uniform alignment of some size goes to HBM as a row image whose rows all begin on multiples of 128
    // bytes (2D copies: free on the way up): the column scan's loads are then aligned (multi_gpu.hip).  Everything
    // else - small inputs, files the geometry walk does not accept - is copied as it is, and the transform itself
    // words what is wrong with it.
    HostBytes e, q;
    if (lay.ok) {
        const size_t dev_size = (size_t)upload_row_image(msa, lay, 0, lay.L, ctx->d_in, ctx->host_tmp, st).bytes;
        msa_image_to_text(ctx->msa, ctx->d_in, dev_size, context_len, ctx->d_eds, ctx->d_seds, e, q, st);
    } else msa_transform_plain(ctx->msa, msa, msa_size, context_len, ctx->d_in, ctx->d_eds, ctx->d_seds, e, q, st);
    give(eds, e);
    give(seds, q);
}

// K column batches; false: this input is not cut (see msa_transform_batched)
bool msa_transform_in_batches(edsx_ctx* ctx, const uint8_t* msa, const MsaLayout& lay, uint32_t context_len, int K,
                              edsx_buf* eds, edsx_buf* seds)
{
    if (!ctx->mini) ctx->mini.reset(new MsaPipeline());
    const SlabWorker w{&ctx->msa, ctx->mini.get(), &ctx->d_in, &ctx->d_eds, &ctx->d_seds, &ctx->d_mini, &ctx->host_tmp};
    HostBytes e, q;
    if (!msa_transform_batched(w, msa, lay, context_len, K, e, q, nullptr)) return false;
    give(eds, e);
    give(seds, q);
    return true;
}

} // namespace

extern "C" {

const char* edsx_version(void) { return "edsx 0.1 (gfx950)"; }

int edsx_ctx_create(int device, edsx_ctx** out)
{
    if (!out) return EDSX_ERR_INVALID_PARAMETER;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count)
        return EDSX_ERR_BUILD_FAILED;           // no GPU: there is no CPU fallback
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return EDSX_ERR_BUILD_FAILED;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return EDSX_ERR_BUILD_FAILED;
    edsx_ctx* c = new (std::nothrow) edsx_ctx();
    if (!c) return EDSX_ERR_BUILD_FAILED;
    c->device = device;
    *out = c;
    return EDSX_OK;
}

void edsx_ctx_destroy(edsx_ctx* ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    delete ctx;
}

const char* edsx_last_error(const edsx_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

void edsx_buf_free(edsx_buf* buf)
{
    if (!buf) return;
    free(buf->data);
    buf->data = nullptr;
    buf->size = 0;
}

int edsx_msa_plan_device(edsx_ctx* ctx, const uint8_t* d_msa, size_t msa_size, uint32_t context_len,
                         void* stream, uint64_t* eds_bytes, uint64_t* seds_bytes)
{
    return guarded(ctx, [&] {
        if (!d_msa || !eds_bytes || !seds_bytes) throw ParamError("null argument");
        ctx->msa.plan(d_msa, msa_size, context_len, static_cast<hipStream_t>(stream), eds_bytes, seds_bytes);
        ctx->last_batches = 1;
    });
}

int edsx_msa_emit_device(edsx_ctx* ctx, uint8_t* d_eds, uint8_t* d_seds, void* stream)
{
    return guarded(ctx, [&] {
        if (!d_eds || !d_seds) throw ParamError("null argument");
        ctx->msa.emit(d_eds, d_seds, static_cast<hipStream_t>(stream));
    });
}

int edsx_msa_last_batches(const edsx_ctx* ctx) { return ctx ? ctx->last_batches : 0; }

int edsx_msa_last_info(const edsx_ctx* ctx, edsx_msa_info* info)
{
    // (after a transform in column batches the pipeline holds the plan of the LAST batch only: no info then)
    if (!ctx || !info || !ctx->msa.planned() || ctx->last_batches > 1) return EDSX_ERR_INVALID_PARAMETER;
    const MsaHdr& h = ctx->msa.header();
    info->n_rows = h.S; info->n_cols = h.L; info->line_width = h.lw ? h.lw : h.L;
    info->n_variant_cols = h.nv; info->n_segments = h.nseg; info->msa_bytes = ctx->msa.msa_bytes();
    info->n_slow_segments = h.slow_n + h.slow_n2;
    return EDSX_OK;
}

int edsx_msa_edge_info(edsx_ctx* ctx, edsx_msa_edges* out)
{
    return guarded(ctx, [&] {
        if (!out) throw ParamError("null argument");
        MsaPipeline::Edges e = ctx->msa.edge_info(nullptr);
        out->n_segments = e.nseg;
        out->first_is_variant = e.fvar; out->first_cols = e.fcols; out->first_eds_bytes = e.feds; out->first_seds_bytes = e.fseds;
        out->last_is_variant = e.lvar; out->last_cols = e.lcols; out->last_eds_bytes = e.leds; out->last_seds_bytes = e.lseds;
    });
}

int edsx_msa_anchor_info(edsx_ctx* ctx, uint64_t min_cols, edsx_msa_anchors* out)
{
    return guarded(ctx, [&] {
        if (!out) throw ParamError("null argument");
        const MsaPipeline::Anchors a = ctx->msa.anchor_info(min_cols, nullptr);
        out->n_segments = a.nseg; out->found = a.found; out->first_seg = a.first_seg; out->last_seg = a.last_seg;
        out->last_col = a.last_col; out->last_eds_bytes = a.last_eds; out->last_seds_bytes = a.last_seds;
        out->first_end = a.first_end; out->first_eds_end = a.first_eds_end; out->first_seds_end = a.first_seds_end;
    });
}

int edsx_msa_copy_columns(edsx_ctx* ctx, uint64_t col0, uint64_t ncols, uint8_t* host_out)
{
    return guarded(ctx, [&] {
        if (!host_out) throw ParamError("null argument");
        ctx->msa.copy_columns(col0, ncols, host_out, nullptr);
    });
}

int edsx_msa_locate_segment(edsx_ctx* ctx, uint64_t col, uint64_t* seg, uint64_t* seg_col, uint64_t* eds_off,
                            uint64_t* seds_off)
{
    return guarded(ctx, [&] {
        if (!seg || !seg_col || !eds_off || !seds_off) throw ParamError("null argument");
        const MsaPipeline::SegLoc r = ctx->msa.locate(col, nullptr);
        *seg = r.seg; *seg_col = r.col; *eds_off = r.eds_off; *seds_off = r.seds_off;
    });
}

int edsx_multi_create(const int* device_ids, int n, int use_rccl, edsx_multi** out)
{
    if (!out) return EDSX_ERR_INVALID_PARAMETER;
    *out = nullptr;
    if (!device_ids || n <= 0) return EDSX_ERR_INVALID_PARAMETER;
    edsx_multi_impl* mi = new (std::nothrow) edsx_multi_impl();
    if (!mi) return EDSX_ERR_BUILD_FAILED;
    try {
        mi->m.reset(new MultiMsa(std::vector<int>(device_ids, device_ids + n), use_rccl != 0));
    } catch (const ParamError&) { delete mi; return EDSX_ERR_INVALID_PARAMETER;
    } catch (const std::exception&) { delete mi; return EDSX_ERR_BUILD_FAILED; }
    *out = reinterpret_cast<edsx_multi*>(mi);
    return EDSX_OK;
}
void edsx_multi_destroy(edsx_multi* m) { delete reinterpret_cast<edsx_multi_impl*>(m); }
const char* edsx_multi_last_error(const edsx_multi* m)
{
    return m ? reinterpret_cast<const edsx_multi_impl*>(m)->err.c_str() : "null handle";
}
int edsx_msa_transform_multi(edsx_multi* m, const uint8_t* msa, size_t msa_size, uint32_t context_len, edsx_buf* eds, edsx_buf* seds)
{
    clear(eds, seds);
    edsx_multi_impl* mi = reinterpret_cast<edsx_multi_impl*>(m);
    if (!mi || !msa || !eds || !seds) return EDSX_ERR_INVALID_PARAMETER;       // (no text: the handle's last one stays)
    return guarded(mi, [&] {
        HostBytes e, s;
        mi->m->transform(msa, msa_size, context_len, e, s);
        give(eds, e);
        give(seds, s);
    });
}
int edsx_multi_last_partition(const edsx_multi* m, int* partitioned, int* chains)
{
    const edsx_multi_impl* mi = reinterpret_cast<const edsx_multi_impl*>(m);
    if (!mi) return EDSX_ERR_INVALID_PARAMETER;
    if (partitioned) *partitioned = mi->m->partitioned() ? 1 : 0;
    if (chains) *chains = mi->m->chains();
    return EDSX_OK;
}

int edsx_vcf_transform_multi(edsx_multi* m, const uint8_t* vcf, size_t vcf_size, const uint8_t* fasta, size_t fasta_size,
                             uint32_t context_len, edsx_buf* eds, edsx_buf* seds, edsx_vcf_stats* stats)
{
    clear(eds, seds);
    zero(stats);
    edsx_multi_impl* mi = reinterpret_cast<edsx_multi_impl*>(m);
    return guarded(mi, [&] {
        if (!eds || !seds || (!vcf && vcf_size) || (!fasta && fasta_size)) throw ParamError("null argument");
        vcf_result([&](HostBytes& e, HostBytes& s, VcfCounters& c) { mi->m->vcf_transform(vcf, vcf_size, fasta, fasta_size, e, s, c); },
                   [&](HostBytes& e, HostBytes& s) { mi->m->leds_merge(e, s, context_len); }, context_len, eds, seds, stats);
    });
}
int edsx_multi_last_vcf(const edsx_multi* m, edsx_vcf_multi_info* out)
{
    const edsx_multi_impl* mi = reinterpret_cast<const edsx_multi_impl*>(m);
    if (!mi || !out) return EDSX_ERR_INVALID_PARAMETER;
    const VcfMultiInfo& v = mi->m->last_vcf();
    out->partitioned = v.partitioned ? 1 : 0;
    out->fasta_windowed = v.fasta_windowed ? 1 : 0;
    out->records_min = v.records_min; out->records_max = v.records_max;
    out->moved_line_bytes = v.moved_line_bytes; out->fasta_h2d_bytes_max = v.fasta_h2d_bytes_max;
    return EDSX_OK;
}

int edsx_leds_merge_multi(edsx_multi* m, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size,
                          uint32_t context_len, int compact, edsx_buf* leds, edsx_buf* seds_out)
{
    clear(leds, seds_out);
    edsx_multi_impl* mi = reinterpret_cast<edsx_multi_impl*>(m);
    return guarded(mi, [&] {
        if (!leds || !seds_out || (!eds && eds_size)) throw ParamError("null argument");
        HostBytes out, sout;
        mi->m->leds_merge_multi(eds, eds_size, seds, seds_size, context_len, compact != 0, out, sout);
        give(leds, out);
        give(seds_out, sout);
    });
}
int edsx_multi_last_merge(const edsx_multi* m, edsx_merge_multi_info* out)
{
    const edsx_multi_impl* mi = reinterpret_cast<const edsx_multi_impl*>(m);
    if (!mi || !out) return EDSX_ERR_INVALID_PARAMETER;
    const MergeMultiInfo& v = mi->m->last_merge();
    out->partitioned = v.partitioned ? 1 : 0;
    out->ranges = v.ranges;
    out->fallback = v.fallback;
    out->range_bytes_min = v.range_bytes_min; out->range_bytes_max = v.range_bytes_max;
    out->eds_h2d_bytes_max = v.eds_h2d_bytes_max; out->seds_h2d_bytes_max = v.seds_h2d_bytes_max;
    return EDSX_OK;
}

void edsx_set_timing(edsx_ctx* ctx, int enabled)
{
    if (!ctx) return;
    ctx->msa.set_timing(enabled != 0);
    ctx->subset.set_timing(enabled != 0);
    ctx->gfa.set_timing(enabled != 0);
    ctx->vcf_export.set_timing(enabled != 0);
    ctx->slice_times.set(enabled != 0);
    ctx->dist_times.set(enabled != 0);
    ctx->ld_times.set(enabled != 0);
    ctx->ibs_times.set(enabled != 0);
    ctx->mosaic_times.set(enabled != 0);
    ctx->div_times.set(enabled != 0);
}
int edsx_get_timing(edsx_ctx* ctx, const char** names, float* total_ms, int* launches, int cap)
{
    if (!ctx) return 0;
    int n = ctx->msa.get_timing(names, total_ms, launches, cap);
    n += ctx->subset.get_timing(names + n, total_ms + n, launches + n, cap - n);
    n += ctx->gfa.get_timing(names + n, total_ms + n, launches + n, cap - n);
    n += ctx->vcf_export.get_timing(names + n, total_ms + n, launches + n, cap - n);
    n += ctx->slice_times.get(names + n, total_ms + n, launches + n, cap - n);
    n += ctx->dist_times.get(names + n, total_ms + n, launches + n, cap - n);
    n += ctx->ld_times.get(names + n, total_ms + n, launches + n, cap - n);
    n += ctx->ibs_times.get(names + n, total_ms + n, launches + n, cap - n);
    n += ctx->mosaic_times.get(names + n, total_ms + n, launches + n, cap - n);
    return n + ctx->div_times.get(names + n, total_ms + n, launches + n, cap - n);
}

int edsx_msa_transform(edsx_ctx* ctx, const uint8_t* msa, size_t msa_size, uint32_t context_len,
                       edsx_buf* eds, edsx_buf* seds)
{
    clear(eds, seds);
    return guarded(ctx, [&] {
        if (!msa || !eds || !seds) throw ParamError("null argument");
        if (msa_size == 0) throw FormatError("Invalid MSA: empty input");
        MsaLayout lay;
        if (msa_size >= ((size_t)1 << 20)) lay = msa_layout(msa, msa_size);
        std::string oom;
        ctx->last_batches = 0;
        try { msa_transform_whole(ctx, msa, msa_size, lay, context_len, eds, seds); ctx->last_batches = 1; return; }
        catch (const OutOfDeviceMemory& ex) { oom = ex.what(); }
        // The alignment and its tables do not fit the device in one piece: column batches, each with the working set of
        // a K-th of the columns (the reference streams an alignment of any size, msa_transforms.cpp:36-90)
        for (int K = 2; K <= 256 && lay.ok; K *= 2) {
            release_msa_buffers(ctx);
            try {
                if (!msa_transform_in_batches(ctx, msa, lay, context_len, K, eds, seds)) break;
                ctx->last_batches = K;
                return;
            } catch (const OutOfDeviceMemory& ex) { oom = ex.what(); }
        }
        release_msa_buffers(ctx);
        throw LimitError("the alignment does not fit the device, in one piece or in column batches (" + oom + ")");
    });
}

int edsx_msa_transform_batched(edsx_ctx* ctx, const uint8_t* msa, size_t msa_size, uint32_t context_len, int batches,
                               edsx_buf* eds, edsx_buf* seds, int* batches_used)
{
    clear(eds, seds);
    if (batches_used) *batches_used = 0;
    return guarded(ctx, [&] {
        if (!msa || !eds || !seds) throw ParamError("null argument");
        if (batches < 1) throw ParamError("edsx_msa_transform_batched: batches must be at least 1");
        if (msa_size == 0) throw FormatError("Invalid MSA: empty input");
        const MsaLayout lay = msa_layout(msa, msa_size);
        ctx->last_batches = 0;
        if (batches > 1 && lay.ok && msa_transform_in_batches(ctx, msa, lay, context_len, batches, eds, seds)) {
            if (batches_used) *batches_used = batches;
            ctx->last_batches = batches;
            return;
        }
        msa_transform_whole(ctx, msa, msa_size, lay, context_len, eds, seds);
        if (batches_used) *batches_used = 1;
        ctx->last_batches = 1;
    });
}

int edsx_leds_merge(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size,
                    uint32_t context_len, int compact, edsx_buf* leds, edsx_buf* seds_out)
{
    clear(leds, seds_out);
    return guarded(ctx, [&] {
        if (!leds || !seds_out || (!eds && eds_size)) throw ParamError("null argument");
        HostBytes out, sout;
        ctx->merge.run(ctx->eds, or_empty(eds), eds_size, seds, seds_size, context_len, compact != 0, out, sout, nullptr);
        give(leds, out);
        give(seds_out, sout);
    });
}

int edsx_eds_stats(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size,
                   uint32_t context_len, edsx_eds_statistics* out)
{
    zero(out);
    return guarded(ctx, [&] {
        if (!out || (!eds && eds_size)) throw ParamError("null argument");
        EdsStats s{};
        ctx->eds.load(or_empty(eds), eds_size, seds, seds_size, seds != nullptr, nullptr);
        eds_stats(ctx->eds, context_len, ctx->stats_acc, s, nullptr);
        out->n_symbols = s.n_symbols; out->n_chars = s.n_chars; out->n_strings = s.n_strings;
        out->num_degenerate_symbols = s.num_degenerate; out->total_change_size = s.total_change_size;
        out->num_common_chars = s.num_common_chars; out->num_empty_strings = s.num_empty_strings;
        out->min_context_length = s.min_context; out->max_context_length = s.max_context;
        out->num_context_blocks = s.num_context_blocks;
        out->avg_context_length = s.num_context_blocks ? (double)s.num_common_chars / (double)s.num_context_blocks : 0.0;   // eds.cpp:428-432
        out->has_sources = s.has_sources; out->num_paths = s.num_paths; out->max_paths_per_string = s.max_paths_per_string;
        out->total_paths = s.total_paths;
        out->avg_paths_per_string = (s.has_sources && s.n_strings) ? (double)s.total_paths / (double)s.n_strings : 0.0;   // eds.cpp:501-503
        out->is_leds = (int)s.is_leds;
    });
}

int edsx_leds_tokenised_on_device(const edsx_ctx* ctx) { return ctx && ctx->eds.tokenised_on_device() ? 1 : 0; }

int edsx_leds_merge_range(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size,
                          uint32_t context_len, int compact, int head_sentinel, int tail_sentinel, edsx_buf* leds,
                          edsx_buf* seds_out, int* head_intact, int* tail_intact)
{
    clear(leds, seds_out);
    if (head_intact) *head_intact = 0;
    if (tail_intact) *tail_intact = 0;
    return guarded(ctx, [&] {
        if (!leds || !seds_out || !head_intact || !tail_intact || (!eds && eds_size)) throw ParamError("null argument");
        HostBytes out, sout;
        MergeShard sh;
        sh.head_sentinel = head_sentinel != 0; sh.tail_sentinel = tail_sentinel != 0;
        ctx->merge.run(ctx->eds, or_empty(eds), eds_size, seds, seds_size, context_len, compact != 0, out, sout, nullptr, &sh);
        *head_intact = sh.head_intact ? 1 : 0;
        *tail_intact = sh.tail_intact ? 1 : 0;
        give(leds, out);
        give(seds_out, sout);
    });
}

int edsx_eds_genpatterns(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, uint64_t count, uint32_t pattern_length,
                         uint64_t seed, edsx_buf* patterns, edsx_buf* witness_pos, edsx_buf* witness_off, edsx_buf* witness_deg)
{
    clear(patterns, witness_pos, witness_off, witness_deg);
    return guarded(ctx, [&] {
        const int nw = (witness_pos != nullptr) + (witness_off != nullptr) + (witness_deg != nullptr);
        if (!patterns || (!eds && eds_size) || (nw != 0 && nw != 3)) throw ParamError("null argument");
        HostBytes out;
        std::vector<u64> wpos, woff;
        std::vector<int32_t> wdeg;
        ctx->query.genpatterns(ctx->eds, or_empty(eds), eds_size, count, pattern_length, seed, out, nw ? &wpos : nullptr,
                               nw ? &woff : nullptr, nw ? &wdeg : nullptr, nullptr);
        if (nw) {
            take_copy(witness_pos, wpos.data(), 8 * wpos.size());
            take_copy(witness_off, woff.data(), 8 * woff.size());
            take_copy(witness_deg, wdeg.data(), 4 * wdeg.size());
        }
        give(patterns, out);
    });
}

int edsx_eds_check_positions(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size,
                             size_t n, const uint64_t* common_pos, const uint64_t* choice_off, const int32_t* choices,
                             const uint64_t* pattern_off, const uint8_t* patterns, int8_t* status_out)
{
    return guarded(ctx, [&] {
        if ((!eds && eds_size) || (n && (!common_pos || !choice_off || !pattern_off || !status_out)) ||
            (n && choice_off[n] && !choices) || (n && pattern_off[n] && !patterns))
            throw ParamError("null argument");
        static_assert(sizeof(u64) == sizeof(uint64_t), "u64");
        ctx->query.check(ctx->eds, or_empty(eds), eds_size, seds, seds_size, n, reinterpret_cast<const u64*>(common_pos),
                         reinterpret_cast<const u64*>(choice_off), choices, reinterpret_cast<const u64*>(pattern_off), patterns,
                         status_out, nullptr);
    });
}

int edsx_eds_locate(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size, size_t n,
                    const uint64_t* pattern_off, const uint8_t* patterns, uint64_t max_hits, uint32_t flags, edsx_buf* hit_off,
                    edsx_buf* hits, edsx_buf* choice_off, edsx_buf* choices, edsx_buf* totals, edsx_buf* pattern_flags)
{
    clear(hit_off, hits, choice_off, choices, totals, pattern_flags);
    return guarded(ctx, [&] {
        if (!hit_off || !hits || !choice_off || !choices || !totals || !pattern_flags || (!eds && eds_size) ||
            (n && (!pattern_off || !patterns)))
            throw ParamError("null argument");
        if (flags & ~EDSX_LOCATE_COMMON_ONLY) throw ParamError("edsx_eds_locate: unknown flag");
        static_assert(sizeof(u64) == sizeof(uint64_t) && sizeof(LocateHit) == sizeof(edsx_locate_hit) &&
                      offsetof(LocateHit, offset) == offsetof(edsx_locate_hit, offset) && LocatePipeline::MAX_CHOICES == EDSX_LOCATE_MAX_CHOICES,
                      "edsx_locate_hit is LocateHit");
        const u64 none = 0;
        LocateOut o;
        ctx->locate.run(ctx->query, ctx->eds, or_empty(eds), eds_size, seds, seds_size, n,
                        n ? reinterpret_cast<const u64*>(pattern_off) : &none, patterns, max_hits,
                        (flags & EDSX_LOCATE_COMMON_ONLY) != 0, o, nullptr);
        take_copy(hit_off, o.hit_off.data(), 8 * o.hit_off.size());
        take_copy(hits, o.hits.data(), sizeof(LocateHit) * o.hits.size());
        take_copy(choice_off, o.choice_off.data(), 8 * o.choice_off.size());
        take_copy(choices, o.choices.data(), 4 * o.choices.size());
        take_copy(totals, o.totals.data(), 8 * o.totals.size());
        take_copy(pattern_flags, o.flags.data(), o.flags.size());
    });
}

int edsx_query_last_info(const edsx_ctx* ctx, edsx_query_info* out)
{
    if (!ctx || !out) return EDSX_ERR_INVALID_PARAMETER;
    const QueryInfo& q = ctx->query.info();
    out->n_symbols = q.n_symbols; out->n_strings = q.n_strings; out->n_chars = q.n_chars;
    out->num_common_chars = q.num_common_chars; out->num_degenerate_strings = q.num_degenerate_strings;
    out->tokenise_ms = q.tokenise_ms; out->tables_ms = q.tables_ms; out->kernel_ms = q.kernel_ms; out->download_ms = q.download_ms;
    return EDSX_OK;
}

int edsx_eds_scan_range(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, uint64_t lo, uint64_t hi, uint32_t context_len,
                        edsx_eds_range_scan* out)
{
    zero(out);
    return guarded(ctx, [&] {
        if (!out || (!eds && eds_size)) throw ParamError("null argument");
        const uint8_t* p = or_empty(eds);
        const EdsRangeScan s = ctx->scan.eds(p, eds_size, text_end(p, eds_size), lo, hi, context_len, nullptr);
        out->ok = s.ok ? 1 : 0;
        out->strings = s.strings;
        out->has_cut = s.has_cut ? 1 : 0;
        out->sym_start = s.sym_start; out->sym_end = s.sym_end; out->strings_before = s.strings_before;
    });
}

int edsx_seds_scan_range(edsx_ctx* ctx, const uint8_t* seds, size_t seds_size, uint64_t lo, uint64_t hi, const uint64_t* ordinals,
                         size_t n_ordinals, int* ok, uint64_t* braces, uint64_t* set_start, uint64_t* set_end)
{
    if (ok) *ok = 0;
    if (braces) *braces = 0;
    return guarded(ctx, [&] {
        if (!ok || !braces || (!seds && seds_size) || (n_ordinals && (!ordinals || !set_start || !set_end)))
            throw ParamError("null argument");
        static_assert(sizeof(u64) == sizeof(uint64_t), "u64");
        u64 b = 0;
        const bool good = ctx->scan.seds_count(or_empty(seds), seds_size, lo, hi, b, nullptr);
        *ok = good ? 1 : 0;
        *braces = b;
        if (good && n_ordinals)
            ctx->scan.seds_locate(reinterpret_cast<const u64*>(ordinals), n_ordinals, reinterpret_cast<u64*>(set_start),
                                  reinterpret_cast<u64*>(set_end), nullptr);
    });
}

int edsx_vcf_tokenised_on_device(const edsx_ctx* ctx) { return ctx && ctx->vcf.tokenised_on_device() ? 1 : 0; }

int edsx_vcf_transform(edsx_ctx* ctx, const uint8_t* vcf, size_t vcf_size, const uint8_t* fasta, size_t fasta_size,
                       uint32_t context_len, edsx_buf* eds, edsx_buf* seds, edsx_vcf_stats* stats)
{
    clear(eds, seds);
    zero(stats);
    return guarded(ctx, [&] {
        if (!eds || !seds || (!vcf && vcf_size) || (!fasta && fasta_size)) throw ParamError("null argument");
        vcf_result([&](HostBytes& e, HostBytes& s, VcfCounters& c) {
                       ctx->vcf.run(or_empty(vcf), vcf_size, or_empty(fasta), fasta_size, e, s, c, nullptr);
                   },
                   [&](HostBytes& e, HostBytes& s) { merge_in_place(ctx, e, s, context_len); }, context_len, eds, seds, stats);
    });
}

// ---- contig sessions (vcf_contig.hip)
struct edsx_vcf_session {
    edsx_ctx* ctx;
    VcfSession s;
    bool z = false;                          // opened on inflated inputs
    GzInfo gz[2];                            // their compressed layer; every call of the session republishes it as the context's last info
    edsx_vcf_session(edsx_ctx* c, const uint8_t* vcf, size_t vcf_n, const uint8_t* fasta, size_t fasta_n)
        : ctx(c), s(vcf, vcf_n, fasta, fasta_n) {}
    edsx_vcf_session(edsx_ctx* c, GzText& vcf, GzText& fasta, bool own, bool ignore_chrom) : ctx(c), s(vcf, fasta, own, ignore_chrom), z(true) {}
    void count_downloads()
    {
        if (!z) return;
        gz[0].text_d2h_bytes = s.vcf_d2h;
        gz[1].text_d2h_bytes = s.fasta_d2h;
        ctx->gz[0] = gz[0]; ctx->gz[1] = gz[1];
    }
};
static_assert(sizeof(edsx_contig) == sizeof(ContigRec) && offsetof(edsx_contig, duplicate) == offsetof(ContigRec, duplicate),
              "edsx_contig is ContigRec");

int edsx_vcf_session_open(edsx_ctx* ctx, const uint8_t* vcf, size_t vcf_size, const uint8_t* fasta, size_t fasta_size,
                          edsx_vcf_session** out)
{
    if (out) *out = nullptr;
    return guarded(ctx, [&] {
        if (!out || (!vcf && vcf_size) || (!fasta && fasta_size)) throw ParamError("null argument");
        std::unique_ptr<edsx_vcf_session> s(new edsx_vcf_session(ctx, or_empty(vcf), vcf_size, or_empty(fasta), fasta_size));
        s->s.open(nullptr);
        *out = s.release();
    });
}

int edsx_vcf_session_contigs(const edsx_vcf_session* s, const edsx_contig** records, size_t* n)
{
    if (!s || !records || !n) return EDSX_ERR_INVALID_PARAMETER;
    *records = reinterpret_cast<const edsx_contig*>(s->s.contigs().data());
    *n = s->s.contigs().size();
    return EDSX_OK;
}

int edsx_vcf_session_find(const edsx_vcf_session* s, const char* name, size_t* index)
{
    if (!s) return EDSX_ERR_INVALID_PARAMETER;
    return guarded(s->ctx, [&] {
        if (!name || !index) throw ParamError("null argument");
        if (!s->s.find(name, *index)) throw ParamError("Contig '" + std::string(name) + "' not found in reference FASTA");
    });
}

int edsx_vcf_session_transform(edsx_vcf_session* s, size_t index, uint32_t context_len, edsx_buf* eds, edsx_buf* seds,
                               edsx_vcf_stats* stats)
{
    clear(eds, seds);
    zero(stats);
    if (!s) return EDSX_ERR_INVALID_PARAMETER;
    edsx_ctx* ctx = s->ctx;
    return guarded(ctx, [&] {
        if (!eds || !seds) throw ParamError("null argument");
        vcf_result([&](HostBytes& e, HostBytes& q, VcfCounters& c) {
                       try { s->s.transform(ctx->vcf, index, e, q, c, nullptr); } catch (...) { s->count_downloads(); throw; }
                       s->count_downloads();
                   },
                   [&](HostBytes& e, HostBytes& q) { merge_in_place(ctx, e, q, context_len); }, context_len, eds, seds, stats);
    });
}

int edsx_vcf_session_info(const edsx_vcf_session* s, edsx_vcf_session_stats* out)
{
    if (!s || !out) return EDSX_ERR_INVALID_PARAMETER;
    out->records_total = s->s.records_total; out->records_without_token = s->s.records_without_token;
    out->records_unknown_contig = s->s.records_unknown;
    out->vcf_h2d_bytes = s->s.vcf_h2d; out->fasta_h2d_bytes = s->s.fasta_h2d;
    out->classified_on_device = s->s.classified_on_device ? 1 : 0;
    return EDSX_OK;
}

int edsx_vcf_session_unknown_contigs(const edsx_vcf_session* s, edsx_buf* text)
{
    clear(text);
    if (!s) return EDSX_ERR_INVALID_PARAMETER;
    return guarded(s->ctx, [&] {
        if (!text) throw ParamError("null argument");
        const std::string& t = s->s.unknown_contigs();
        take_copy(text, t.data(), t.size());
    });
}

void edsx_vcf_session_close(edsx_vcf_session* s)
{
    if (!s) return;
    (void)hipSetDevice(s->ctx->device);
    delete s;
}

int edsx_vcf_transform_contig(edsx_ctx* ctx, const uint8_t* vcf, size_t vcf_size, const uint8_t* fasta, size_t fasta_size,
                              const char* contig, uint32_t context_len, edsx_buf* eds, edsx_buf* seds, edsx_vcf_stats* stats)
{
    clear(eds, seds);
    zero(stats);
    edsx_vcf_session* s = nullptr;
    return in_session(edsx_vcf_session_open(ctx, vcf, vcf_size, fasta, fasta_size, &s), s, edsx_vcf_session_close, [&] {
        size_t index = 0;
        const int rc = edsx_vcf_session_find(s, contig, &index);
        return rc == EDSX_OK ? edsx_vcf_session_transform(s, index, context_len, eds, seds, stats) : rc;
    });
}

// ---- compressed input (bgzf_device.hip, inflate.hpp)
int edsx_gz_probe(const uint8_t* data, size_t size, int* kind)
{
    if (!kind || (!data && size)) return EDSX_ERR_INVALID_PARAMETER;
    *kind = (int)gz::gz_probe(data, size);
    return EDSX_OK;
}

int edsx_bgzf_index(const uint8_t* data, size_t size, edsx_buf* blocks, uint64_t* text_size)
{
    clear(blocks);
    if (text_size) *text_size = 0;
    if (!blocks || !text_size || (!data && size)) return EDSX_ERR_INVALID_PARAMETER;
    static_assert(sizeof(edsx_bgzf_block) == sizeof(gz::BgzfBlock) && offsetof(edsx_bgzf_block, isize) == offsetof(gz::BgzfBlock, isize),
                  "edsx_bgzf_block is BgzfBlock");
    try {
        std::vector<gz::BgzfBlock> tab;
        u64 n = 0;
        if (gz::gz_walk(data, size, n, [&](const gz::BgzfBlock& b) { tab.push_back(b); }) != gz::GZ_BGZF) return EDSX_ERR_INVALID_FORMAT;
        take_copy(blocks, tab.data(), tab.size() * sizeof(gz::BgzfBlock));
        *text_size = n;
    } catch (...) { return EDSX_ERR_BUILD_FAILED; }
    return EDSX_OK;
}

int edsx_gz_inflate(edsx_ctx* ctx, const uint8_t* data, size_t size, edsx_buf* text)
{
    clear(text);
    return guarded(ctx, [&] {
        if (!text || (!data && size)) throw ParamError("null argument");
        ctx->gz[0] = GzInfo(); ctx->gz[1] = GzInfo();
        GzText t;
        gz_open(or_empty(data), size, "input", t, ctx->gz[0], nullptr);
        HostBytes out;
        out.take(t.n);
        if (t.on_device) PinnedDownload::copy(out.data, t.dev.ptr, t.n, nullptr);     // (the caller asked for the text: not a text_d2h of a transform)
        else if (t.n) std::memcpy(out.data, t.on_host ? t.host.data() : t.plain, t.n);
        give(text, out);
    });
}

int edsx_gz_last_info(const edsx_ctx* ctx, int which, edsx_gz_info* out)
{
    if (!ctx || !out || which < 0 || which > 1) return EDSX_ERR_INVALID_PARAMETER;
    static_assert(sizeof(edsx_gz_info) == sizeof(GzInfo), "edsx_gz_info is GzInfo");
    std::memcpy(out, &ctx->gz[which], sizeof(*out));
    return EDSX_OK;
}

namespace {

// inflate both inputs (the VCF's errors first) and build the session on them
edsx_vcf_session* open_z(edsx_ctx* ctx, const uint8_t* vcf, size_t vcf_size, const uint8_t* fasta, size_t fasta_size, bool own, bool ignore_chrom)
{
    ctx->gz[0] = GzInfo(); ctx->gz[1] = GzInfo();
    GzText v, f;
    gz_open(or_empty(vcf), vcf_size, "VCF", v, ctx->gz[0], nullptr);
    gz_open(or_empty(fasta), fasta_size, "FASTA", f, ctx->gz[1], nullptr);
    std::unique_ptr<edsx_vcf_session> s(new edsx_vcf_session(ctx, v, f, own, ignore_chrom));
    s->gz[0] = ctx->gz[0]; s->gz[1] = ctx->gz[1];
    try { s->s.open(nullptr); } catch (...) { s->count_downloads(); throw; }
    s->count_downloads();
    return s.release();
}

} // namespace

int edsx_vcf_session_open_z(edsx_ctx* ctx, const uint8_t* vcf, size_t vcf_size, const uint8_t* fasta, size_t fasta_size,
                            edsx_vcf_session** out)
{
    if (out) *out = nullptr;
    return guarded(ctx, [&] {
        if (!out || (!vcf && vcf_size) || (!fasta && fasta_size)) throw ParamError("null argument");
        *out = open_z(ctx, vcf, vcf_size, fasta, fasta_size, true, false);
    });
}

int edsx_vcf_session_contig_name(const edsx_vcf_session* s, size_t index, const char** name, size_t* len)
{
    if (!s || !name || !len || index >= s->s.contigs().size()) return EDSX_ERR_INVALID_PARAMETER;
    const std::string& n = s->s.name(index);
    *name = n.data(); *len = n.size();
    return EDSX_OK;
}

int edsx_vcf_transform_z(edsx_ctx* ctx, const uint8_t* vcf, size_t vcf_size, const uint8_t* fasta, size_t fasta_size, const char* contig,
                         uint32_t context_len, edsx_buf* eds, edsx_buf* seds, edsx_vcf_stats* stats)
{
    clear(eds, seds);
    zero(stats);
    edsx_vcf_session* s = nullptr;
    const int opened = guarded(ctx, [&] {
        if (!eds || !seds || (!vcf && vcf_size) || (!fasta && fasta_size)) throw ParamError("null argument");
        s = open_z(ctx, vcf, vcf_size, fasta, fasta_size, false, contig == nullptr);
    });
    return in_session(opened, s, edsx_vcf_session_close, [&] {
        size_t index = 0;
        const int rc = contig ? edsx_vcf_session_find(s, contig, &index) : EDSX_OK;
        return rc == EDSX_OK ? edsx_vcf_session_transform(s, index, context_len, eds, seds, stats) : rc;
    });
}

// ---- path sessions (path_device.hip)
struct edsx_paths_session {
    edsx_ctx* ctx;
    PathPipeline p;
};

int edsx_paths_open(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size,
                    edsx_paths_session** out)
{
    if (out) *out = nullptr;
    return guarded(ctx, [&] {
        if (!out || (!eds && eds_size)) throw ParamError("null argument");
        std::unique_ptr<edsx_paths_session> s(new edsx_paths_session{ctx, {}});
        s->p.open(or_empty(eds), eds_size, seds, seds_size, nullptr);
        *out = s.release();
    });
}

int edsx_paths_info(const edsx_paths_session* s, edsx_paths_info_t* out)
{
    if (!s || !out) return EDSX_ERR_INVALID_PARAMETER;
    const PathInfo& i = s->p.info();
    out->n_symbols = i.n_symbols; out->n_strings = i.n_strings; out->n_chars = i.n_chars; out->num_paths = i.num_paths;
    out->n_choice_symbols = i.n_choice_symbols; out->tokenised_on_device = i.tokenised_on_device ? 1 : 0;
    return EDSX_OK;
}

int edsx_paths_lengths(edsx_paths_session* s, const uint64_t* ids, size_t n, uint64_t* length, uint64_t* missing)
{
    if (!s) return EDSX_ERR_INVALID_PARAMETER;
    return guarded(s->ctx, [&] {
        if (n && (!ids || !length)) throw ParamError("null argument");
        static_assert(sizeof(u64) == sizeof(uint64_t), "u64");
        s->p.lengths(reinterpret_cast<const u64*>(ids), n, reinterpret_cast<u64*>(length), reinterpret_cast<u64*>(missing), nullptr);
    });
}

int edsx_paths_spell(edsx_paths_session* s, const uint64_t* ids, size_t n, const char* const* names, const char* prefix,
                     uint64_t line_width, edsx_buf* fasta, uint64_t* missing)
{
    clear(fasta);
    if (!s) return EDSX_ERR_INVALID_PARAMETER;
    return guarded(s->ctx, [&] {
        if (!fasta || (n && !ids)) throw ParamError("null argument");
        std::vector<u64> all;
        if (n == 0) {                                            // every path
            if (names) throw ParamError("names need an explicit list of path ids");
            all.resize(s->p.info().num_paths);
            for (size_t k = 0; k < all.size(); k++) all[k] = k + 1;
        }
        if (names) for (size_t k = 0; k < n; k++) if (!names[k]) throw ParamError("null argument");
        HostBytes out;
        s->p.spell(n ? reinterpret_cast<const u64*>(ids) : all.data(), n ? n : all.size(), names, prefix, line_width, out,
                   reinterpret_cast<u64*>(missing), nullptr);
        give(fasta, out);
    });
}

int edsx_paths_last_timing(const edsx_paths_session* s, edsx_paths_timing* out)
{
    if (!s || !out) return EDSX_ERR_INVALID_PARAMETER;
    const PathTiming& t = s->p.timing();
    out->tokenise_ms = t.tokenise_ms; out->choose_ms = t.choose_ms; out->scan_ms = t.scan_ms; out->copy_ms = t.copy_ms;
    out->download_ms = t.download_ms; out->bytes_written = t.bytes_written;
    return EDSX_OK;
}

void edsx_paths_close(edsx_paths_session* s)
{
    if (!s) return;
    (void)hipSetDevice(s->ctx->device);
    delete s;
}

int edsx_eds_spell_paths(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size,
                         const uint64_t* ids, size_t n, const char* const* names, const char* prefix, uint64_t line_width,
                         edsx_buf* fasta, uint64_t* missing)
{
    clear(fasta);
    edsx_paths_session* s = nullptr;
    return in_session(edsx_paths_open(ctx, eds, eds_size, seds, seds_size, &s), s, edsx_paths_close,
                      [&] { return edsx_paths_spell(s, ids, n, names, prefix, line_width, fasta, missing); });
}

int edsx_eds_subset(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size, const uint64_t* ids,
                    size_t n, int keep_ids, edsx_buf* eds_out, edsx_buf* seds_out, edsx_subset_info* info)
{
    clear(eds_out, seds_out);
    zero(info);
    return guarded(ctx, [&] {
        if (!eds_out || !seds_out || (!eds && eds_size) || (n && !ids)) throw ParamError("null argument");
        static_assert(sizeof(SubsetInfo) == sizeof(edsx_subset_info) &&
                      offsetof(SubsetInfo, common_runs_merged) == offsetof(edsx_subset_info, common_runs_merged),
                      "edsx_subset_info is SubsetInfo");
        HostBytes e, s;
        SubsetInfo si;
        ctx->subset.run(ctx->eds, or_empty(eds), eds_size, seds, seds_size, reinterpret_cast<const u64*>(ids), n, keep_ids != 0, e, s,
                        si, nullptr);
        if (info) std::memcpy(info, &si, sizeof(si));
        give(eds_out, e);
        give(seds_out, s);
    });
}

// ---- eds2gfa (gfa_device.hip; the P lines: path_device.hip)
int edsx_eds_gfa_graph(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, uint64_t max_links, edsx_buf* gfa, edsx_gfa_info* info)
{
    clear(gfa);
    zero(info);
    return guarded(ctx, [&] {
        if (!gfa || (!eds && eds_size)) throw ParamError("null argument");
        static_assert(offsetof(edsx_gfa_info, tokenised_on_device) == sizeof(GfaInfo), "edsx_gfa_info begins with GfaInfo");
        HostBytes g;
        GfaInfo gi;
        try { ctx->gfa.run(ctx->eds, or_empty(eds), eds_size, nullptr, 0, max_links, g, gi, nullptr); }
        catch (const ParamError&) {                              // the link limit: the counts are known
            if (info) { std::memcpy(info, &gi, sizeof(gi)); info->tokenised_on_device = ctx->eds.tokenised_on_device() ? 1 : 0; }
            throw;
        }
        if (info) { std::memcpy(info, &gi, sizeof(gi)); info->tokenised_on_device = ctx->eds.tokenised_on_device() ? 1 : 0; }
        give(gfa, g);
    });
}

int edsx_paths_gfa_walks(edsx_paths_session* s, const uint64_t* ids, size_t n, const char* const* names, const char* prefix,
                         edsx_buf* lines, uint64_t* missing, uint64_t* steps)
{
    clear(lines);
    if (!s) return EDSX_ERR_INVALID_PARAMETER;
    return guarded(s->ctx, [&] {
        if (!lines || (n && !ids)) throw ParamError("null argument");
        std::vector<u64> all;
        if (n == 0) {                                            // every path
            if (names) throw ParamError("names need an explicit list of path ids");
            all.resize(s->p.info().num_paths);
            for (size_t k = 0; k < all.size(); k++) all[k] = k + 1;
        }
        if (names) for (size_t k = 0; k < n; k++) if (!names[k]) throw ParamError("null argument");
        HostBytes out;
        s->p.walks(n ? reinterpret_cast<const u64*>(ids) : all.data(), n ? n : all.size(), names, prefix, out,
                   reinterpret_cast<u64*>(missing), reinterpret_cast<u64*>(steps), nullptr);
        give(lines, out);
    });
}

int edsx_eds_gfa(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size, uint64_t max_links,
                 const char* prefix, edsx_buf* gfa, edsx_gfa_info* info)
{
    clear(gfa);
    zero(info);
    if (!seds) return edsx_eds_gfa_graph(ctx, eds, eds_size, max_links, gfa, info);
    edsx_paths_session* s = nullptr;                             // first: a text that does not match its sources is an error
    return in_session(edsx_paths_open(ctx, eds, eds_size, seds, seds_size, &s), s, edsx_paths_close, [&] {
        edsx_buf graph{nullptr, 0}, lines{nullptr, 0};
        int rc = edsx_eds_gfa_graph(ctx, eds, eds_size, max_links, &graph, info);
        if (rc == EDSX_OK) rc = edsx_paths_gfa_walks(s, nullptr, 0, nullptr, prefix, &lines, nullptr, nullptr);
        if (rc == EDSX_OK)
            rc = guarded(ctx, [&] {
                if (!gfa) throw ParamError("null argument");
                gfa->data = HostBytes::alloc(graph.size + lines.size);
                gfa->size = graph.size + lines.size;
                if (graph.size) std::memcpy(gfa->data, graph.data, graph.size);
                if (lines.size) std::memcpy(gfa->data + graph.size, lines.data, lines.size);
            });
        edsx_buf_free(&graph);
        edsx_buf_free(&lines);
        return rc;
    });
}

// ---- eds2msa (path_device.hip)
int edsx_paths_align_info(edsx_paths_session* s, edsx_align_info* out)
{
    zero(out);
    if (!s) return EDSX_ERR_INVALID_PARAMETER;
    return guarded(s->ctx, [&] {
        if (!out) throw ParamError("null argument");
        static_assert(sizeof(AlignInfo) == sizeof(edsx_align_info) && offsetof(AlignInfo, num_paths) == offsetof(edsx_align_info, num_paths),
                      "edsx_align_info is AlignInfo");
        std::memcpy(out, &s->p.align_info(nullptr), sizeof(*out));
    });
}

int edsx_paths_align(edsx_paths_session* s, const uint64_t* ids, size_t n, const char* const* names, const char* prefix,
                     uint64_t line_width, int gap, uint64_t max_bytes, edsx_buf* fasta, uint64_t* missing)
{
    clear(fasta);
    if (!s) return EDSX_ERR_INVALID_PARAMETER;
    return guarded(s->ctx, [&] {
        if (!fasta || (n && !ids)) throw ParamError("null argument");
        std::vector<u64> all;
        if (n == 0) {                                            // every path
            if (names) throw ParamError("names need an explicit list of path ids");
            all.resize(s->p.info().num_paths);
            for (size_t k = 0; k < all.size(); k++) all[k] = k + 1;
        }
        if (names) for (size_t k = 0; k < n; k++) if (!names[k]) throw ParamError("null argument");
        if (gap < 0 || gap > 255) throw ParamError("Gap character is not usable in an alignment");
        HostBytes out;
        s->p.align(n ? reinterpret_cast<const u64*>(ids) : all.data(), n ? n : all.size(), names, prefix, line_width,
                   gap ? (uint8_t)gap : (uint8_t)'-', max_bytes, out, reinterpret_cast<u64*>(missing), nullptr);
        give(fasta, out);
    });
}

int edsx_eds_msa(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size, const uint64_t* ids,
                 size_t n, const char* const* names, const char* prefix, uint64_t line_width, int gap, uint64_t max_bytes,
                 edsx_buf* fasta, uint64_t* missing, edsx_align_info* info)
{
    clear(fasta);
    zero(info);
    edsx_paths_session* s = nullptr;
    return in_session(edsx_paths_open(ctx, eds, eds_size, seds, seds_size, &s), s, edsx_paths_close, [&] {
        edsx_align_info ai;
        const int rc = edsx_paths_align_info(s, &ai);
        if (rc != EDSX_OK) return rc;
        if (info) *info = ai;
        return edsx_paths_align(s, ids, n, names, prefix, line_width, gap, max_bytes, fasta, missing);
    });
}

// ---- edsparser-lift (path_device.hip, lift_core.hpp)
static_assert(sizeof(LiftSite) == sizeof(edsx_lift_site) && offsetof(LiftSite, common_pos) == offsetof(edsx_lift_site, common_pos),
              "edsx_lift_site is LiftSite");

int edsx_paths_lift_sites(edsx_paths_session* s, size_t n, const uint64_t* path, const uint64_t* pos, edsx_lift_site* site,
                          uint8_t* status)
{
    if (!s) return EDSX_ERR_INVALID_PARAMETER;
    return guarded(s->ctx, [&] {
        if (n && (!path || !pos || !site || !status)) throw ParamError("null argument");
        s->p.lift(n, reinterpret_cast<const u64*>(path), reinterpret_cast<const u64*>(pos), nullptr, nullptr,
                  reinterpret_cast<LiftSite*>(site), nullptr, status, nullptr);
    });
}

int edsx_paths_lift_place(edsx_paths_session* s, size_t n, const uint64_t* symbol, const uint64_t* string, const uint64_t* offset,
                          const uint64_t* dst_path, uint64_t* dst_pos, uint8_t* status)
{
    if (!s) return EDSX_ERR_INVALID_PARAMETER;
    return guarded(s->ctx, [&] {
        if (n && (!symbol || !string || !offset || !dst_path || !dst_pos || !status)) throw ParamError("null argument");
        const LiftColumns sites{reinterpret_cast<const u64*>(symbol), reinterpret_cast<const u64*>(string), reinterpret_cast<const u64*>(offset)};
        s->p.lift(n, nullptr, nullptr, &sites, reinterpret_cast<const u64*>(dst_path), nullptr, reinterpret_cast<u64*>(dst_pos),
                  status, nullptr);
    });
}

int edsx_paths_lift(edsx_paths_session* s, size_t n, const uint64_t* src_path, const uint64_t* src_pos, const uint64_t* dst_path,
                    uint64_t* dst_pos, uint8_t* status, edsx_lift_site* site)
{
    if (!s) return EDSX_ERR_INVALID_PARAMETER;
    return guarded(s->ctx, [&] {
        if (n && (!src_path || !src_pos || !dst_path || !dst_pos || !status)) throw ParamError("null argument");
        s->p.lift(n, reinterpret_cast<const u64*>(src_path), reinterpret_cast<const u64*>(src_pos), nullptr,
                  reinterpret_cast<const u64*>(dst_path), reinterpret_cast<LiftSite*>(site), reinterpret_cast<u64*>(dst_pos), status, nullptr);
    });
}

int edsx_eds_lift(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size, size_t n,
                  const uint64_t* src_path, const uint64_t* src_pos, const uint64_t* dst_path, uint64_t* dst_pos, uint8_t* status,
                  edsx_lift_site* site)
{
    edsx_paths_session* s = nullptr;
    return in_session(edsx_paths_open(ctx, eds, eds_size, seds, seds_size, &s), s, edsx_paths_close,
                      [&] { return edsx_paths_lift(s, n, src_path, src_pos, dst_path, dst_pos, status, site); });
}

// ---- edsparser-slice (slice_device.hip, slice_core.hpp)
static_assert(sizeof(SliceRegion) == sizeof(edsx_slice_region) && offsetof(SliceRegion, seds_len) == offsetof(edsx_slice_region, seds_len),
              "edsx_slice_region is SliceRegion");
static_assert(EDSX_SLICE_RANGE == slice::RANGE, "EDSX_SLICE_RANGE");

int edsx_paths_slice(edsx_paths_session* s, size_t n, const uint64_t* path, const uint64_t* start, const uint64_t* end,
                     uint64_t max_bytes, edsx_buf* eds_out, edsx_buf* seds_out, edsx_slice_region* region, uint8_t* status)
{
    clear(eds_out, seds_out);
    if (!s) return EDSX_ERR_INVALID_PARAMETER;
    return guarded(s->ctx, [&] {
        if (!eds_out || !seds_out || (n && (!path || !start || !end || !status))) throw ParamError("null argument");
        HostBytes e, q;
        s->p.slice(n, reinterpret_cast<const u64*>(path), reinterpret_cast<const u64*>(start), reinterpret_cast<const u64*>(end), max_bytes,
                   e, q, reinterpret_cast<SliceRegion*>(region), status, &s->ctx->slice_times, nullptr);
        give(eds_out, e);
        give(seds_out, q);
    });
}

int edsx_eds_slice(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size, size_t n,
                   const uint64_t* path, const uint64_t* start, const uint64_t* end, uint64_t max_bytes, edsx_buf* eds_out,
                   edsx_buf* seds_out, edsx_slice_region* region, uint8_t* status)
{
    clear(eds_out, seds_out);
    edsx_paths_session* s = nullptr;
    return in_session(edsx_paths_open(ctx, eds, eds_size, seds, seds_size, &s), s, edsx_paths_close,
                      [&] { return edsx_paths_slice(s, n, path, start, end, max_bytes, eds_out, seds_out, region, status); });
}

// ---- edsparser-dist (dist_device.hip, dist_core.hpp)
static_assert(sizeof(DistInfo) == sizeof(edsx_dist_info) && offsetof(DistInfo, chunks) == offsetof(edsx_dist_info, chunks),
              "edsx_dist_info is DistInfo");
static_assert(EDSX_DIST_COLUMNS == dist::COLUMNS && EDSX_DIST_STRINGS == dist::STRINGS, "EDSX_DIST_*");

int edsx_paths_distances(edsx_paths_session* s, const uint64_t* ids, size_t n, int metric, uint64_t max_bytes, uint64_t* matrix,
                         uint64_t* missing, edsx_dist_info* info)
{
    zero(info);
    if (!s) return EDSX_ERR_INVALID_PARAMETER;
    return guarded(s->ctx, [&] {
        if (n && !ids) throw ParamError("null argument");
        std::vector<u64> all;
        if (n == 0) {                                            // every path
            all.resize(s->p.info().num_paths);
            for (size_t k = 0; k < all.size(); k++) all[k] = k + 1;
        }
        const size_t K = n ? n : all.size();
        DistInfo di;                                             // (a null matrix: refused behind the limit check, which needs none)
        try {
            s->p.distances(n ? reinterpret_cast<const u64*>(ids) : all.data(), K, metric, max_bytes, reinterpret_cast<u64*>(matrix),
                           reinterpret_cast<u64*>(missing), di, &s->ctx->dist_times, nullptr);
        } catch (const LimitError&) {                            // the budget: the geometry is known
            if (info) std::memcpy(info, &di, sizeof(di));
            throw;
        }
        if (info) std::memcpy(info, &di, sizeof(di));
    });
}

int edsx_eds_distances(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size, const uint64_t* ids,
                       size_t n, int metric, uint64_t max_bytes, uint64_t* matrix, uint64_t* missing, edsx_dist_info* info)
{
    zero(info);
    edsx_paths_session* s = nullptr;
    return in_session(edsx_paths_open(ctx, eds, eds_size, seds, seds_size, &s), s, edsx_paths_close,
                      [&] { return edsx_paths_distances(s, ids, n, metric, max_bytes, matrix, missing, info); });
}

// ---- edsparser-ld (ld_device.hip, ld_core.hpp)
static_assert(sizeof(LdInfo) == sizeof(edsx_ld_info) && offsetof(LdInfo, tiles) == offsetof(edsx_ld_info, tiles), "edsx_ld_info is LdInfo");
static_assert(sizeof(LdOpts) == sizeof(edsx_ld_opts) && offsetof(LdOpts, max_pairs) == offsetof(edsx_ld_opts, max_pairs), "edsx_ld_opts is LdOpts");
static_assert(sizeof(LdPair) == sizeof(edsx_ld_pair) && offsetof(LdPair, r2) == offsetof(edsx_ld_pair, r2), "edsx_ld_pair is LdPair");
static_assert(sizeof(LdAllele) == sizeof(edsx_ld_allele) && offsetof(LdAllele, present) == offsetof(edsx_ld_allele, present),
              "edsx_ld_allele is LdAllele");

int edsx_paths_ld(edsx_paths_session* s, const uint64_t* ids, size_t n, const edsx_ld_opts* opts, edsx_buf* pairs, edsx_buf* alleles,
                  edsx_ld_info* info)
{
    clear(pairs, alleles);
    zero(info);
    if (!s) return EDSX_ERR_INVALID_PARAMETER;
    return guarded(s->ctx, [&] {
        if (!pairs || !opts || (n && !ids)) throw ParamError("null argument");
        LdOpts o;
        std::memcpy(&o, opts, sizeof(o));
        LdInfo li;
        HostBytes p, a;
        try {
            s->p.ld(reinterpret_cast<const u64*>(ids), n, o, p, alleles ? &a : nullptr, li, &s->ctx->ld_times, nullptr);
        } catch (...) {                                          // as far as the call got
            if (info) std::memcpy(info, &li, sizeof(li));
            throw;
        }
        if (info) std::memcpy(info, &li, sizeof(li));
        give(pairs, p);
        if (alleles) give(alleles, a);
    });
}

int edsx_eds_ld(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size, const uint64_t* ids, size_t n,
                const edsx_ld_opts* opts, edsx_buf* pairs, edsx_buf* alleles, edsx_ld_info* info)
{
    clear(pairs, alleles);
    zero(info);
    edsx_paths_session* s = nullptr;
    return in_session(edsx_paths_open(ctx, eds, eds_size, seds, seds_size, &s), s, edsx_paths_close,
                      [&] { return edsx_paths_ld(s, ids, n, opts, pairs, alleles, info); });
}

// ---- edsparser-ibs (ibs_device.hip, ibs_core.hpp)
static_assert(sizeof(IbsInfo) == sizeof(edsx_ibs_info) && offsetof(IbsInfo, segments) == offsetof(edsx_ibs_info, segments), "edsx_ibs_info is IbsInfo");
static_assert(sizeof(IbsSegment) == sizeof(edsx_ibs_segment) && offsetof(IbsSegment, column_end) == offsetof(edsx_ibs_segment, column_end),
              "edsx_ibs_segment is IbsSegment");

int edsx_paths_ibs(edsx_paths_session* s, const uint64_t* ids, size_t n, uint64_t min_sites, uint64_t min_columns, uint64_t max_segments,
                   edsx_buf* segments, edsx_buf* pair_off, edsx_ibs_info* info)
{
    clear(segments, pair_off);
    zero(info);
    if (!s) return EDSX_ERR_INVALID_PARAMETER;
    return guarded(s->ctx, [&] {
        if (!segments || !pair_off || (n && !ids)) throw ParamError("null argument");
        IbsInfo ii;
        HostBytes sg, po;
        try {
            s->p.ibs(reinterpret_cast<const u64*>(ids), n, min_sites, min_columns, max_segments, sg, po, ii, &s->ctx->ibs_times, nullptr);
        } catch (...) {                                          // as far as the call got
            if (info) std::memcpy(info, &ii, sizeof(ii));
            throw;
        }
        if (info) std::memcpy(info, &ii, sizeof(ii));
        give(segments, sg);
        give(pair_off, po);
    });
}

int edsx_eds_ibs(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size, const uint64_t* ids, size_t n,
                 uint64_t min_sites, uint64_t min_columns, uint64_t max_segments, edsx_buf* segments, edsx_buf* pair_off, edsx_ibs_info* info)
{
    clear(segments, pair_off);
    zero(info);
    edsx_paths_session* s = nullptr;
    return in_session(edsx_paths_open(ctx, eds, eds_size, seds, seds_size, &s), s, edsx_paths_close,
                      [&] { return edsx_paths_ibs(s, ids, n, min_sites, min_columns, max_segments, segments, pair_off, info); });
}

// ---- edsparser-mosaic (mosaic_device.hip, mosaic_core.hpp)
static_assert(sizeof(MosaicInfo) == sizeof(edsx_mosaic_info) && offsetof(MosaicInfo, switches) == offsetof(edsx_mosaic_info, switches),
              "edsx_mosaic_info is MosaicInfo");
static_assert(sizeof(MosaicSegment) == sizeof(edsx_mosaic_segment) && offsetof(MosaicSegment, column_end) == offsetof(edsx_mosaic_segment, column_end),
              "edsx_mosaic_segment is MosaicSegment");

int edsx_paths_mosaic(edsx_paths_session* s, const uint64_t* targets, size_t nt, const uint64_t* donors, size_t nd, uint64_t max_segments,
                      edsx_buf* segments, edsx_buf* target_off, edsx_mosaic_info* info)
{
    clear(segments, target_off);
    zero(info);
    if (!s) return EDSX_ERR_INVALID_PARAMETER;
    return guarded(s->ctx, [&] {
        if (!segments || !target_off || (nt && !targets) || (nd && !donors)) throw ParamError("null argument");
        MosaicInfo mi;
        HostBytes sg, to;
        try {
            s->p.mosaic(reinterpret_cast<const u64*>(targets), nt, reinterpret_cast<const u64*>(donors), nd, max_segments, sg, to, mi,
                        &s->ctx->mosaic_times, nullptr);
        } catch (...) {                                          // as far as the call got
            if (info) std::memcpy(info, &mi, sizeof(mi));
            throw;
        }
        if (info) std::memcpy(info, &mi, sizeof(mi));
        give(segments, sg);
        give(target_off, to);
    });
}

int edsx_eds_mosaic(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size, const uint64_t* targets,
                    size_t nt, const uint64_t* donors, size_t nd, uint64_t max_segments, edsx_buf* segments, edsx_buf* target_off,
                    edsx_mosaic_info* info)
{
    clear(segments, target_off);
    zero(info);
    edsx_paths_session* s = nullptr;
    return in_session(edsx_paths_open(ctx, eds, eds_size, seds, seds_size, &s), s, edsx_paths_close,
                      [&] { return edsx_paths_mosaic(s, targets, nt, donors, nd, max_segments, segments, target_off, info); });
}

// ---- edsparser-diversity (div_device.hip, div_core.hpp)
static_assert(sizeof(DivInfo) == sizeof(edsx_div_info) && offsetof(DivInfo, extent) == offsetof(edsx_div_info, extent), "edsx_div_info is DivInfo");
static_assert(sizeof(DivOpts) == sizeof(edsx_div_opts) && offsetof(DivOpts, max_windows) == offsetof(edsx_div_opts, max_windows),
              "edsx_div_opts is DivOpts");
static_assert(sizeof(DivWindow) == sizeof(edsx_div_window) && offsetof(DivWindow, rank_end) == offsetof(edsx_div_window, rank_end),
              "edsx_div_window is DivWindow");
static_assert(sizeof(DivGroup) == sizeof(edsx_div_group) && offsetof(DivGroup, present) == offsetof(edsx_div_group, present),
              "edsx_div_group is DivGroup");
static_assert(sizeof(DivPair) == sizeof(edsx_div_pair) && offsetof(DivPair, comp) == offsetof(edsx_div_pair, comp), "edsx_div_pair is DivPair");
static_assert(EDSX_DIV_SYMBOLS == diversity::SYMBOLS && EDSX_DIV_COLUMNS == diversity::COLUMNS && EDSX_DIV_MAX_GROUPS == diversity::MAX_GROUPS,
              "EDSX_DIV_*");

int edsx_paths_diversity(edsx_paths_session* s, const uint64_t* group_off, const uint64_t* group_ids, size_t n_groups, const edsx_div_opts* opts,
                         edsx_buf* windows, edsx_buf* groups, edsx_buf* pairs, edsx_buf* sfs, edsx_div_info* info)
{
    clear(windows, groups, pairs, sfs);
    zero(info);
    if (!s) return EDSX_ERR_INVALID_PARAMETER;
    return guarded(s->ctx, [&] {
        if (!windows || !groups || !pairs || !opts || (n_groups && (!group_off || (group_off[n_groups] && !group_ids))))
            throw ParamError("null argument");
        DivOpts o;
        std::memcpy(&o, opts, sizeof(o));
        DivInfo di;
        HostBytes w, g, p, f;
        try {
            s->p.diversity(reinterpret_cast<const u64*>(group_off), reinterpret_cast<const u64*>(group_ids), n_groups, o, w, g, p, sfs ? &f : nullptr,
                           di, &s->ctx->div_times, nullptr);
        } catch (...) {                                          // as far as the call got
            if (info) std::memcpy(info, &di, sizeof(di));
            throw;
        }
        if (info) std::memcpy(info, &di, sizeof(di));
        give(windows, w);
        give(groups, g);
        give(pairs, p);
        if (sfs) give(sfs, f);
    });
}

int edsx_eds_diversity(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size, const uint64_t* group_off,
                       const uint64_t* group_ids, size_t n_groups, const edsx_div_opts* opts, edsx_buf* windows, edsx_buf* groups,
                       edsx_buf* pairs, edsx_buf* sfs, edsx_div_info* info)
{
    clear(windows, groups, pairs, sfs);
    zero(info);
    edsx_paths_session* s = nullptr;
    return in_session(edsx_paths_open(ctx, eds, eds_size, seds, seds_size, &s), s, edsx_paths_close,
                      [&] { return edsx_paths_diversity(s, group_off, group_ids, n_groups, opts, windows, groups, pairs, sfs, info); });
}

// ---- eds2vcf (vcf_export_device.hip)
int edsx_eds_vcf(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size,
                 const edsx_vcf_export_opts* opts, edsx_buf* vcf, edsx_buf* ref_fasta, edsx_vcf_export_info* info)
{
    clear(vcf, ref_fasta);
    zero(info);
    return guarded(ctx, [&] {
        if (!vcf || (!eds && eds_size) || (opts && opts->n_names && !opts->names)) throw ParamError("null argument");
        static_assert(offsetof(edsx_vcf_export_info, tokenised_on_device) == sizeof(VcfExportInfo),
                      "edsx_vcf_export_info begins with VcfExportInfo");
        VcfExportOpts o;
        if (opts) {
            if (opts->chrom) o.chrom = opts->chrom;
            if (opts->prefix) o.prefix = opts->prefix;
            o.ref_path = opts->ref_path; o.line_width = opts->line_width; o.max_bytes = opts->max_bytes;
            o.names = opts->names; o.n_names = opts->names ? opts->n_names : 0;
            for (size_t k = 0; k < o.n_names; k++) if (!o.names[k]) throw ParamError("null argument");
        }
        HostBytes v, f;
        VcfExportInfo vi;
        auto put_info = [&] {
            if (info) { std::memcpy(info, &vi, sizeof(vi)); info->tokenised_on_device = ctx->eds.tokenised_on_device() ? 1 : 0; }
        };
        try { ctx->vcf_export.run(ctx->eds, or_empty(eds), eds_size, seds, seds_size, o, v, ref_fasta ? &f : nullptr, vi, nullptr); }
        catch (const LimitError&) { put_info(); throw; }         // the byte limit: the counts are known
        put_info();
        give(vcf, v);
        if (ref_fasta) give(ref_fasta, f);
    });
}

int edsx_vcf_index(edsx_ctx* ctx, const uint8_t* vcf, size_t vcf_size, edsx_buf* pos, edsx_buf* reflen, edsx_buf* line_off,
                   edsx_buf* line_len, edsx_vcf_stats* stats)
{
    clear(pos, reflen, line_off, line_len);
    zero(stats);
    return guarded(ctx, [&] {
        if (!pos || !reflen || !line_off || !line_len || (!vcf && vcf_size)) throw ParamError("null argument");
        std::vector<u64> p, r, lo, ll;
        VcfCounters c;
        if (!ctx->vcf.index_device(or_empty(vcf), vcf_size, nullptr, p, r, lo, ll, c))   // plain text: on the GPU
            vcf_index(or_empty(vcf), vcf_size, p, r, lo, ll, c);
        put(stats, c, false);
        take_copy(pos, p.data(), 8 * p.size());
        take_copy(reflen, r.data(), 8 * r.size());
        take_copy(line_off, lo.data(), 8 * lo.size());
        take_copy(line_len, ll.data(), 8 * ll.size());
    });
}

int edsx_vcf_sort_order(const uint64_t* pos, size_t n, uint32_t* order_out)
{
    if ((!pos || !order_out) && n) return EDSX_ERR_INVALID_PARAMETER;
    if (n >= 0xffffffffull) return EDSX_ERR_INVALID_PARAMETER;
    static_assert(sizeof(u64) == sizeof(uint64_t), "u64");
    try { vcf_sort_order(reinterpret_cast<const u64*>(pos), n, order_out); } catch (...) { return EDSX_ERR_BUILD_FAILED; }
    return EDSX_OK;
}

int edsx_vcf_transform_range(edsx_ctx* ctx, const uint8_t* vcf, size_t vcf_size, const uint8_t* fasta, size_t fasta_size,
                             uint64_t cur0, uint64_t next_start, edsx_buf* eds, edsx_buf* seds, edsx_vcf_stats* stats)
{
    clear(eds, seds);
    zero(stats);
    return guarded(ctx, [&] {
        if (!eds || !seds || (!vcf && vcf_size) || (!fasta && fasta_size)) throw ParamError("null argument");
        HostBytes e, s;
        VcfCounters c;
        VcfRange range;
        range.presorted = true; range.cur0 = cur0; range.next_start = next_start;
        ctx->vcf.run(or_empty(vcf), vcf_size, or_empty(fasta), fasta_size, e, s, c, nullptr, range);
        put(stats, c, true);
        give(eds, e);
        give(seds, s);
    });
}

int edsx_genrandomeds(edsx_ctx* ctx, uint64_t total_bp, double variability, uint32_t min_alt, uint32_t max_alt,
                      uint32_t var_len_max, double snp_ratio, const char* alphabet, uint64_t min_context, uint64_t seed,
                      edsx_buf* eds, edsx_buf* seds, uint64_t* n_sites)
{
    clear(eds, seds);
    return guarded(ctx, [&] {
        if (!eds || !seds || !alphabet) throw ParamError("null argument");
        GenParams gp{};
        gp.total_bp = total_bp; gp.variability = variability; gp.min_alt = min_alt; gp.max_alt = max_alt;
        gp.var_len_max = var_len_max; gp.snp_ratio = snp_ratio; gp.min_context = min_context; gp.seed = seed;
        const size_t an = std::strlen(alphabet);
        if (an > 64) throw ParamError("Alphabet of more than 64 characters is not supported by this build");
        gp.alpha_n = (u32)an;
        std::memcpy(gp.alphabet, alphabet, an);
        HostBytes e, s;
        u64 sites = 0;
        ctx->gen.run(gp, e, s, sites, nullptr);
        if (n_sites) *n_sites = sites;
        give(eds, e);
        give(seds, s);
    });
}

int edsx_genvcf(edsx_ctx* ctx, uint64_t ref_len, uint64_t n_records, uint32_t n_samples, uint64_t seed, edsx_buf* vcf, edsx_buf* fasta)
{
    clear(vcf, fasta);
    return guarded(ctx, [&] {
        if (!vcf || !fasta) throw ParamError("null argument");
        HostBytes v, f;
        ctx->genvcf.run(ref_len, n_records, n_samples, seed, v, f, nullptr);
        give(vcf, v);
        give(fasta, f);
    });
}

size_t edsx_msa_synth_size(uint32_t n_rows, uint64_t n_cols) { return synth_size(n_rows, n_cols); }

int edsx_msa_synth_device(edsx_ctx* ctx, uint8_t* d_out, size_t capacity, uint32_t n_rows,
                          uint64_t col0, uint64_t n_cols, double variant_fraction, uint64_t seed,
                          void* stream, size_t* written)
{
    return guarded(ctx, [&] {
        if (!d_out || n_rows < 1 || n_cols < 1) throw ParamError("bad synthetic alignment geometry");
        size_t need = synth_size(n_rows, n_cols);
        if (capacity < need) throw ParamError("output buffer too small for the synthetic alignment");
        ctx->synth_desc.ensure(8 * (size_t)n_cols);
        synth_generate(d_out, ctx->synth_desc.as<u64>(), n_rows, col0, n_cols, variant_fraction, seed,
                       static_cast<hipStream_t>(stream));
        EDSX_HIP(hipGetLastError());
        if (written) *written = need;
    });
}

size_t edsx_msa_synth_size_aligned(uint32_t n_rows, uint64_t n_cols, uint32_t row_align) { return synth_size_aligned(n_rows, n_cols, row_align); }

int edsx_msa_synth_device_aligned(edsx_ctx* ctx, uint8_t* d_out, size_t capacity, uint32_t n_rows, uint64_t col0, uint64_t n_cols,
                                  double variant_fraction, uint64_t seed, uint32_t row_align, void* stream, size_t* written)
{
    return guarded(ctx, [&] {
        if (!d_out || n_rows < 1 || n_cols < 1 || n_rows > 99999) throw ParamError("bad synthetic alignment geometry");
        if (row_align > 1 && (row_align & (row_align - 1))) throw ParamError("row alignment must be a power of two");
        size_t need = synth_size_aligned(n_rows, n_cols, row_align);
        if (capacity < need) throw ParamError("output buffer too small for the synthetic alignment");
        ctx->synth_desc.ensure(8 * (size_t)n_cols);
        synth_generate(d_out, ctx->synth_desc.as<u64>(), n_rows, col0, n_cols, variant_fraction, seed,
                       static_cast<hipStream_t>(stream), row_align);
        EDSX_HIP(hipGetLastError());
        if (written) *written = need;
    });
}

} // extern "C"
