// edsparser::eds_to_leds_{linear,cartesian} + is_leds over the C ABI.
// Reference: src/cpp/lib/transforms/eds_transforms.cpp:313-373, :381-426, :439-468.
#include "edsparser/transforms/eds_transforms.hpp"
#include "device.hpp"

#include <algorithm>
#include <cstring>

namespace edsparser {

static void run_merge(std::istream& input, std::ostream& output, Length context_length, std::istream* phasing_input,
                      std::ostream* phasing_output, bool compact)
{
    if (context_length == 0)
        throw std::invalid_argument("context_length must be > 0 for l-EDS transformation");
    std::string eds = detail::slurp(input);
    std::string seds;
    if (phasing_input) seds = detail::slurp(*phasing_input);
    edsx_ctx* ctx = detail::context();
    detail::Buf out, sout;
    int rc = edsx_leds_merge(ctx, reinterpret_cast<const uint8_t*>(eds.data()), eds.size(),
                             phasing_input ? reinterpret_cast<const uint8_t*>(seds.data()) : nullptr, seds.size(),
                             context_length, compact ? 1 : 0, &out.b, &sout.b);
    if (rc != EDSX_OK) detail::throw_status(rc, ctx);
    output.write(reinterpret_cast<const char*>(out.b.data), static_cast<std::streamsize>(out.b.size));
    if (phasing_output && phasing_input)
        phasing_output->write(reinterpret_cast<const char*>(sout.b.data), static_cast<std::streamsize>(sout.b.size));
}

void eds_to_leds_linear(std::istream& input, std::ostream& output, Length context_length, std::istream* phasing_input,
                        std::ostream* phasing_output, size_t /*num_threads*/, bool compact)
{
    run_merge(input, output, context_length, phasing_input, phasing_output, compact);
}

void eds_to_leds_cartesian(std::istream& input, std::ostream& output, Length context_length, size_t /*num_threads*/,
                           bool compact)
{
    run_merge(input, output, context_length, nullptr, nullptr, compact);
}

void eds_to_fasta(std::istream& eds_in, std::istream& seds_in, std::ostream& out, const std::vector<int>& paths,
                  size_t line_width, const std::vector<std::string>* names, std::vector<size_t>* missing)
{
    if (names && names->size() != paths.size()) throw std::invalid_argument("eds_to_fasta: one name per requested path");
    const std::string eds = detail::slurp(eds_in), seds = detail::slurp(seds_in);
    std::vector<uint64_t> ids;
    for (int p : paths) ids.push_back(p < 0 ? 0 : static_cast<uint64_t>(p));      // (0 is out of range as well)
    std::vector<const char*> np;
    if (names) for (const auto& s : *names) np.push_back(s.c_str());
    edsx_ctx* ctx = detail::context();
    edsx_paths_session* s = nullptr;
    int rc = edsx_paths_open(ctx, reinterpret_cast<const uint8_t*>(eds.data()), eds.size(),
                             reinterpret_cast<const uint8_t*>(seds.data()), seds.size(), &s);
    if (rc != EDSX_OK) detail::throw_status(rc, ctx);
    edsx_paths_info_t info;
    edsx_paths_info(s, &info);
    std::vector<uint64_t> miss(ids.empty() ? info.num_paths : ids.size());
    detail::Buf fasta;
    rc = edsx_paths_spell(s, ids.data(), ids.size(), names && !np.empty() ? np.data() : nullptr, nullptr, line_width, &fasta.b,
                          miss.data());
    edsx_paths_close(s);
    if (rc != EDSX_OK) detail::throw_status(rc, ctx);
    out.write(reinterpret_cast<const char*>(fasta.b.data), static_cast<std::streamsize>(fasta.b.size));
    if (missing) missing->assign(miss.begin(), miss.end());
}

void eds_to_msa(std::istream& eds_in, std::istream& seds_in, std::ostream& out, const std::vector<int>& paths, size_t line_width,
                const std::vector<std::string>* names, const std::string& prefix, char gap, size_t max_bytes, AlignInfo* info)
{
    if (names && names->size() != paths.size()) throw std::invalid_argument("eds_to_msa: one name per requested path");
    const std::string eds = detail::slurp(eds_in), seds = detail::slurp(seds_in);
    std::vector<uint64_t> ids;
    for (int p : paths) ids.push_back(p < 0 ? 0 : static_cast<uint64_t>(p));      // (0 is out of range as well)
    std::vector<const char*> np;
    if (names) for (const auto& s : *names) np.push_back(s.c_str());
    edsx_ctx* ctx = detail::context();
    edsx_paths_session* s = nullptr;
    int rc = edsx_paths_open(ctx, reinterpret_cast<const uint8_t*>(eds.data()), eds.size(),
                             reinterpret_cast<const uint8_t*>(seds.data()), seds.size(), &s);
    if (rc != EDSX_OK) detail::throw_status(rc, ctx);
    edsx_align_info ai;
    rc = edsx_paths_align_info(s, &ai);
    std::vector<uint64_t> miss(ids.empty() ? ai.num_paths : ids.size());
    detail::Buf fasta;
    // (a gap of 0 would mean the default: hand the C ABI a value it refuses instead)
    if (rc == EDSX_OK)
        rc = edsx_paths_align(s, ids.data(), ids.size(), names && !np.empty() ? np.data() : nullptr, prefix.c_str(), line_width,
                              gap ? static_cast<unsigned char>(gap) : 256, max_bytes, &fasta.b, miss.data());
    edsx_paths_close(s);
    if (rc != EDSX_OK) detail::throw_status(rc, ctx);
    out.write(reinterpret_cast<const char*>(fasta.b.data), static_cast<std::streamsize>(fasta.b.size));
    if (info) {
        info->n_symbols = ai.n_symbols; info->n_columns = ai.n_columns; info->n_zero_width_symbols = ai.n_zero_width_symbols;
        info->widest_symbol = ai.widest_symbol; info->num_paths = ai.num_paths;
        info->missing.assign(miss.begin(), miss.end());
    }
}

std::vector<LiftResult> lift_positions(std::istream& eds_in, std::istream& seds_in, const std::vector<LiftQuery>& queries)
{
    const std::string eds = detail::slurp(eds_in), seds = detail::slurp(seds_in);
    const size_t n = queries.size();
    std::vector<uint64_t> src(n), pos(n), dst(n), out(n);
    for (size_t q = 0; q < n; q++) { src[q] = queries[q].src_path; pos[q] = queries[q].src_pos; dst[q] = queries[q].dst_path; }
    std::vector<uint8_t> status(n);
    std::vector<edsx_lift_site> site(n);
    edsx_ctx* ctx = detail::context();
    const int rc = edsx_eds_lift(ctx, reinterpret_cast<const uint8_t*>(eds.data()), eds.size(),
                                 reinterpret_cast<const uint8_t*>(seds.data()), seds.size(), n, src.data(), pos.data(), dst.data(),
                                 out.data(), status.data(), site.data());
    if (rc != EDSX_OK) detail::throw_status(rc, ctx);
    std::vector<LiftResult> res(n);
    for (size_t q = 0; q < n; q++) {
        res[q].dst_pos = out[q]; res[q].symbol = site[q].symbol; res[q].string = site[q].string; res[q].offset = site[q].offset;
        res[q].column = site[q].column; res[q].common_pos = site[q].common_pos;
        res[q].status = static_cast<LiftStatus>(status[q]);
    }
    return res;
}

PathDistances path_distances(std::istream& eds_in, std::istream& seds_in, const std::vector<int>& paths, DistanceMetric metric)
{
    const std::string eds = detail::slurp(eds_in), seds = detail::slurp(seds_in);
    std::vector<uint64_t> ids;
    for (int p : paths) ids.push_back(p < 0 ? 0 : static_cast<uint64_t>(p));      // (0 is out of range as well)
    edsx_ctx* ctx = detail::context();
    edsx_paths_session* s = nullptr;
    int rc = edsx_paths_open(ctx, reinterpret_cast<const uint8_t*>(eds.data()), eds.size(),
                             reinterpret_cast<const uint8_t*>(seds.data()), seds.size(), &s);
    if (rc != EDSX_OK) detail::throw_status(rc, ctx);
    edsx_paths_info_t pi;
    edsx_paths_info(s, &pi);
    PathDistances d;
    d.K = ids.empty() ? pi.num_paths : ids.size();
    std::vector<uint64_t> miss(d.K);
    edsx_dist_info di;
    try { d.matrix.resize(d.K * d.K); } catch (...) { edsx_paths_close(s); throw; }
    rc = edsx_paths_distances(s, ids.data(), ids.size(), static_cast<int>(metric), 0, d.matrix.data(), miss.data(), &di);
    edsx_paths_close(s);
    if (rc != EDSX_OK) detail::throw_status(rc, ctx);
    d.units = di.units; d.variable_units = di.variable_units; d.class_columns = di.class_columns;
    d.missing.assign(miss.begin(), miss.end());
    return d;
}

PathLd path_ld(std::istream& eds_in, std::istream& seds_in, const std::vector<int>& paths, const LdOptions& options)
{
    const std::string eds = detail::slurp(eds_in), seds = detail::slurp(seds_in);
    std::vector<uint64_t> ids;
    for (int p : paths) ids.push_back(p < 0 ? 0 : static_cast<uint64_t>(p));      // (0 is out of range as well)
    edsx_ctx* ctx = detail::context();
    edsx_ld_opts lo;
    lo.window = options.window; lo.min_r2 = options.min_r2; lo.min_count = options.min_count;
    lo.all_strings = options.all_strings ? 1 : 0; lo.max_pairs = options.max_pairs;
    edsx_buf pb{nullptr, 0}, ab{nullptr, 0};
    edsx_ld_info li;
    const int rc = edsx_eds_ld(ctx, reinterpret_cast<const uint8_t*>(eds.data()), eds.size(), reinterpret_cast<const uint8_t*>(seds.data()),
                               seds.size(), ids.data(), ids.size(), &lo, &pb, &ab, &li);
    if (rc != EDSX_OK) detail::throw_status(rc, ctx);
    PathLd d;
    static_assert(sizeof(LdPair) == sizeof(edsx_ld_pair) && sizeof(LdAllele) == sizeof(edsx_ld_allele), "the records of edsx_paths_ld");
    try {
        d.pairs.resize(li.pairs);
        d.alleles.resize(li.alleles);
    } catch (...) { edsx_buf_free(&pb); edsx_buf_free(&ab); throw; }
    if (li.pairs) std::memcpy(d.pairs.data(), pb.data, sizeof(LdPair) * li.pairs);
    if (li.alleles) std::memcpy(d.alleles.data(), ab.data, sizeof(LdAllele) * li.alleles);
    edsx_buf_free(&pb);
    edsx_buf_free(&ab);
    d.paths = li.paths; d.choice_symbols = li.choice_symbols; d.candidate_pairs = li.candidate_pairs; d.undefined_pairs = li.undefined_pairs;
    return d;
}

PathIbs path_ibs(std::istream& eds_in, std::istream& seds_in, const std::vector<int>& paths, const IbsOptions& options)
{
    const std::string eds = detail::slurp(eds_in), seds = detail::slurp(seds_in);
    std::vector<uint64_t> ids;
    for (int p : paths) ids.push_back(p < 0 ? 0 : static_cast<uint64_t>(p));      // (0 is out of range as well)
    edsx_ctx* ctx = detail::context();
    edsx_buf sb{nullptr, 0}, ob{nullptr, 0};
    edsx_ibs_info ii;
    const int rc = edsx_eds_ibs(ctx, reinterpret_cast<const uint8_t*>(eds.data()), eds.size(), reinterpret_cast<const uint8_t*>(seds.data()),
                                seds.size(), ids.data(), ids.size(), options.min_sites, options.min_columns, options.max_segments, &sb, &ob, &ii);
    if (rc != EDSX_OK) detail::throw_status(rc, ctx);
    PathIbs d;
    static_assert(sizeof(IbsSegment) == sizeof(edsx_ibs_segment), "the records of edsx_paths_ibs");
    try {
        d.segments.resize(ii.segments);
        d.pair_off.resize(ob.size / 8);
    } catch (...) { edsx_buf_free(&sb); edsx_buf_free(&ob); throw; }
    if (ii.segments) std::memcpy(d.segments.data(), sb.data, sizeof(IbsSegment) * ii.segments);
    if (ob.size) std::memcpy(d.pair_off.data(), ob.data, ob.size);
    edsx_buf_free(&sb);
    edsx_buf_free(&ob);
    d.paths = ii.paths; d.choice_symbols = ii.choice_symbols; d.candidate_segments = ii.candidate_segments;
    return d;
}

PathMosaic path_mosaic(std::istream& eds_in, std::istream& seds_in, const std::vector<int>& targets, const std::vector<int>& donors,
                       const MosaicOptions& options)
{
    const std::string eds = detail::slurp(eds_in), seds = detail::slurp(seds_in);
    std::vector<uint64_t> tids, dids;
    for (int p : targets) tids.push_back(p < 0 ? 0 : static_cast<uint64_t>(p));      // (0 is out of range as well)
    for (int p : donors) dids.push_back(p < 0 ? 0 : static_cast<uint64_t>(p));
    edsx_ctx* ctx = detail::context();
    edsx_buf sb{nullptr, 0}, ob{nullptr, 0};
    edsx_mosaic_info mi;
    const int rc = edsx_eds_mosaic(ctx, reinterpret_cast<const uint8_t*>(eds.data()), eds.size(), reinterpret_cast<const uint8_t*>(seds.data()),
                                   seds.size(), tids.data(), tids.size(), dids.data(), dids.size(), options.max_segments, &sb, &ob, &mi);
    if (rc != EDSX_OK) detail::throw_status(rc, ctx);
    PathMosaic d;
    static_assert(sizeof(MosaicSegment) == sizeof(edsx_mosaic_segment), "the records of edsx_paths_mosaic");
    try {
        d.segments.resize(mi.segments);
        d.target_off.resize(ob.size / 8);
    } catch (...) { edsx_buf_free(&sb); edsx_buf_free(&ob); throw; }
    if (mi.segments) std::memcpy(d.segments.data(), sb.data, sizeof(MosaicSegment) * mi.segments);
    if (ob.size) std::memcpy(d.target_off.data(), ob.data, ob.size);
    edsx_buf_free(&sb);
    edsx_buf_free(&ob);
    d.targets = mi.targets; d.donors = mi.donors; d.choice_symbols = mi.choice_symbols;
    d.private_segments = mi.private_segments; d.private_symbols = mi.private_symbols; d.switches = mi.switches;
    return d;
}

PathDiversity path_diversity(std::istream& eds_in, std::istream& seds_in, const std::vector<std::vector<int>>& groups, const DiversityOptions& options)
{
    const std::string eds = detail::slurp(eds_in), seds = detail::slurp(seds_in);
    std::vector<uint64_t> off(1, 0), ids;
    for (const auto& g : groups) {
        for (int p : g) ids.push_back(p < 0 ? 0 : static_cast<uint64_t>(p));      // (0 is out of range as well)
        off.push_back(ids.size());
    }
    edsx_ctx* ctx = detail::context();
    edsx_div_opts o;
    o.unit = static_cast<int>(options.unit); o.size = options.size; o.step = options.step; o.max_windows = options.max_windows;
    detail::Buf wb, gb, pb, fb;
    edsx_div_info di;
    const int rc = edsx_eds_diversity(ctx, reinterpret_cast<const uint8_t*>(eds.data()), eds.size(), reinterpret_cast<const uint8_t*>(seds.data()),
                                      seds.size(), off.data(), ids.data(), groups.size(), &o, &wb.b, &gb.b, &pb.b, options.sfs ? &fb.b : nullptr, &di);
    if (rc != EDSX_OK) detail::throw_status(rc, ctx);
    PathDiversity d;
    static_assert(sizeof(DiversityWindow) == sizeof(edsx_div_window) && sizeof(DiversityGroup) == sizeof(edsx_div_group) &&
                  sizeof(DiversityPair) == sizeof(edsx_div_pair), "the records of edsx_paths_diversity");
    d.windows.resize(wb.b.size / sizeof(DiversityWindow));
    d.groups.resize(gb.b.size / sizeof(DiversityGroup));
    d.pairs.resize(pb.b.size / sizeof(DiversityPair));
    if (wb.b.size) std::memcpy(d.windows.data(), wb.b.data, wb.b.size);
    if (gb.b.size) std::memcpy(d.groups.data(), gb.b.data, gb.b.size);
    if (pb.b.size) std::memcpy(d.pairs.data(), pb.b.data, pb.b.size);
    d.n_groups = di.groups; d.paths = di.paths; d.choice_symbols = di.choice_symbols; d.n_pairs = di.pairs; d.extent = di.extent;
    for (const auto& g : groups) {                               // K_g: the distinct ids
        std::vector<int> u(g);
        std::sort(u.begin(), u.end());
        d.group_paths.push_back(static_cast<uint64_t>(std::unique(u.begin(), u.end()) - u.begin()));
    }
    if (groups.empty()) d.group_paths.push_back(di.paths);
    if (options.sfs) {
        const uint64_t* f = reinterpret_cast<const uint64_t*>(fb.b.data);
        size_t at = 0;
        for (uint64_t K : d.group_paths) {
            const size_t n = fb.b.size ? K + 1 : 0;
            d.sfs.emplace_back(f + at, f + at + n);
            at += n;
        }
    }
    return d;
}

void eds_subset(std::istream& eds_in, std::istream& seds_in, std::ostream& eds_out, std::ostream& seds_out,
                const std::vector<int>& paths, bool keep_ids, SubsetInfo* info)
{
    const std::string eds = detail::slurp(eds_in), seds = detail::slurp(seds_in);
    std::vector<uint64_t> ids;
    for (int p : paths) ids.push_back(p < 0 ? 0 : static_cast<uint64_t>(p));      // (0 is out of range as well)
    edsx_ctx* ctx = detail::context();
    detail::Buf e, s;
    edsx_subset_info si;
    const int rc = edsx_eds_subset(ctx, reinterpret_cast<const uint8_t*>(eds.data()), eds.size(),
                                   reinterpret_cast<const uint8_t*>(seds.data()), seds.size(), ids.data(), ids.size(),
                                   keep_ids ? 1 : 0, &e.b, &s.b, &si);
    if (rc != EDSX_OK) detail::throw_status(rc, ctx);
    eds_out.write(reinterpret_cast<const char*>(e.b.data), static_cast<std::streamsize>(e.b.size));
    seds_out.write(reinterpret_cast<const char*>(s.b.data), static_cast<std::streamsize>(s.b.size));
    if (info) {
        info->symbols_in = si.symbols_in; info->symbols_out = si.symbols_out; info->strings_in = si.strings_in;
        info->strings_out = si.strings_out; info->chars_in = si.chars_in; info->chars_out = si.chars_out;
        info->paths_in = si.paths_in; info->paths_out = si.paths_out; info->symbols_removed = si.symbols_removed;
        info->common_runs_merged = si.common_runs_merged;
    }
}

void eds_to_gfa(std::istream& eds_in, std::istream* seds_in, std::ostream& gfa, const std::vector<int>& paths,
                const std::vector<std::string>* names, const std::string& prefix, size_t max_links, GfaInfo* info)
{
    if (!seds_in && (!paths.empty() || names)) throw std::invalid_argument("eds_to_gfa: paths and names need sources");
    if (names && (names->size() != paths.size() || paths.empty())) throw std::invalid_argument("eds_to_gfa: one name per requested path");
    const std::string eds = detail::slurp(eds_in), seds = seds_in ? detail::slurp(*seds_in) : std::string();
    edsx_ctx* ctx = detail::context();
    edsx_paths_session* s = nullptr;
    int rc = EDSX_OK;
    if (seds_in) {                                               // first: a text that does not match its sources writes nothing
        rc = edsx_paths_open(ctx, reinterpret_cast<const uint8_t*>(eds.data()), eds.size(),
                             reinterpret_cast<const uint8_t*>(seds.data()), seds.size(), &s);
        if (rc != EDSX_OK) detail::throw_status(rc, ctx);
    }
    detail::Buf graph, lines;
    edsx_gfa_info gi;
    rc = edsx_eds_gfa_graph(ctx, reinterpret_cast<const uint8_t*>(eds.data()), eds.size(), max_links, &graph.b, &gi);
    std::vector<uint64_t> miss, steps;
    if (rc == EDSX_OK && s) {
        std::vector<uint64_t> ids;
        for (int p : paths) ids.push_back(p < 0 ? 0 : static_cast<uint64_t>(p));  // (0 is out of range as well)
        std::vector<const char*> np;
        if (names) for (const auto& n : *names) np.push_back(n.c_str());
        edsx_paths_info_t pi;
        edsx_paths_info(s, &pi);
        miss.resize(ids.empty() ? pi.num_paths : ids.size());
        steps.resize(miss.size());
        rc = edsx_paths_gfa_walks(s, ids.data(), ids.size(), np.empty() ? nullptr : np.data(), prefix.c_str(), &lines.b, miss.data(),
                                  steps.data());
    }
    edsx_paths_close(s);
    if (rc != EDSX_OK) detail::throw_status(rc, ctx);
    gfa.write(reinterpret_cast<const char*>(graph.b.data), static_cast<std::streamsize>(graph.b.size));
    gfa.write(reinterpret_cast<const char*>(lines.b.data), static_cast<std::streamsize>(lines.b.size));
    if (info) {
        info->n_symbols = gi.n_symbols; info->n_strings = gi.n_strings; info->n_segments = gi.n_segments;
        info->n_empty_strings = gi.n_empty_strings; info->n_open_symbols = gi.n_open_symbols; info->n_links = gi.n_links;
        info->header_bytes = gi.header_bytes; info->segment_bytes = gi.segment_bytes; info->link_bytes = gi.link_bytes;
        info->missing.assign(miss.begin(), miss.end());
        info->steps.assign(steps.begin(), steps.end());
    }
}

bool is_leds(const EDS& eds, Length context_length)
{
    if (context_length == 0) return true;
    const auto& deg = eds.get_is_degenerate();
    const size_t n = eds.length();
    for (size_t i = 0; i < n; ++i) {
        if (!deg[i]) {
            Length len = eds.get_string_length(eds.get_metadata().cum_set_sizes[i]);
            if (i > 0 && i + 1 < n && len < context_length) return false;
        }
        if (i + 1 < n && deg[i] && deg[i + 1]) return false;
    }
    return true;
}

} // namespace edsparser
