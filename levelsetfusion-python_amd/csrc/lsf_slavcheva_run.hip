// A whole KillingFusion-style optimize() call of a whole volume -- a fixed iteration count or the reference's default
// threshold-terminated loop --, enqueued by the LIBRARY in two host calls
// (include/lsf_hip.h: lsf_state_run_begin / lsf_state_run_finish).  Reference loop: nonrigid_opt/slavcheva/
// slavcheva_optimizer2d.py:354-388 -- one Python iteration of which is ONE kernel launch here; caller shape
// run_hierarchical_optimizer3d_multipair.py:403-432 (a loop of such calls over independent pairs).
//
// The two functions issue the launches of lsf_state_prepare, lsf_state_pack_needed / lsf_state_pack,
// lsf_band_list_fill_prepared, lsf_slavcheva_state_iteration x K and lsf_state_finalize_listed in the order the Python engine
// issues them, on the caller's stream -- results are those launches' results, bit for bit.  Two things differ on the device:
// with a rows buffer a FIXED count's iteration launches end in record rows and one launch makes the records behind the last
// of them (lsf_state_run_finish_rows: the energies in another, fixed, order of adds), and the records' used words are
// gathered by the finalize pass's combine kernel instead of a launch of their own.  What changes most is the host side: K + 8 foreign calls, their argument marshalling and three tensor-level read-backs become two calls
// that run without the interpreter lock (ctypes releases it), so that a second pair's call can be enqueued by another
// host thread meanwhile (experiment/multipair.run_pairs with several optimizers).
#include "lsf_device.h"

#include <cstring>

using namespace lsf;

namespace {

// the four used words of every slot of every record (a record is 8 slots 4 KiB apart) and, behind them, the 16 doubles of
// the convergence statistics, gathered for ONE copy to the host
__global__ __launch_bounds__(kBlock) void records_used_words_kernel(const long long* __restrict__ records,
                                                                    const long long* __restrict__ statistics16,
                                                                    long long* __restrict__ out, int n_slots, int tail) {
    const int k = blockIdx.x * kBlock + threadIdx.x;  // (slot, word), then (tail != 0) the statistics
    if (k < n_slots * 4) out[k] = records[(long long)(k >> 2) * (sizeof(lsf_record_slot) / 8) + (k & 3)];
    else if (tail && k < n_slots * 4 + 16) out[k] = statistics16 ? statistics16[k - n_slots * 4] : 0ll;
}

// Fixed-count calls whose launches ended in record rows (lsf_device.h: wave_reduce_store_row): ONE workgroup per iteration
// combines that iteration's rows_per_iteration rows -- all its launches' -- into slot 0 of records[iteration] and zeroes
// the used words of the other slots, so that the finalize guard, the used-words gather and lsf_records_decode see a record
// as the atomics leave it.  A fixed association (thread t takes rows t, t + kBlock, ...; lanes by wave_sum_f64; the four
// waves in ascending order): the same bits on every run.
__global__ __launch_bounds__(kBlock) void records_from_rows_kernel(const RecordRow* __restrict__ rows,
                                                                   unsigned rows_per_iteration,
                                                                   lsf_iteration_record* __restrict__ records) {
    const RecordRow* mine = rows + (size_t)blockIdx.x * rows_per_iteration;
    unsigned long long best = 0ull;
    double sums[3] = {0.0, 0.0, 0.0};
    for (unsigned r = threadIdx.x; r < rows_per_iteration; r += kBlock) {
        const RecordRow row = mine[r];
        best = row.max_packed > best ? row.max_packed : best;
        sums[0] += row.data;
        sums[1] += row.smoothing;
        sums[2] += row.level_set;
    }
    __shared__ unsigned long long s_max[kBlock / kWave];
    __shared__ double s_sum[3][kBlock / kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    best = wave_max_u64(best);
#pragma unroll
    for (int j = 0; j < 3; ++j) sums[j] = wave_sum_f64(sums[j]);
    if (lane == 0) {
        s_max[wave] = best;
#pragma unroll
        for (int j = 0; j < 3; ++j) s_sum[j][wave] = sums[j];
    }
    __syncthreads();
    lsf_iteration_record* record = records + blockIdx.x;
    if (threadIdx.x == 0) {
        unsigned long long m = 0ull;
        double t[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < kBlock / kWave; ++k) {
            m = s_max[k] > m ? s_max[k] : m;
#pragma unroll
            for (int j = 0; j < 3; ++j) t[j] += s_sum[j][k];
        }
        record->slot[0].max_packed = m;
        record->slot[0].data_energy = t[0];
        record->slot[0].smoothing_energy = t[1];
        record->slot[0].level_set_energy = t[2];
    } else if (threadIdx.x < LSF_RECORD_SLOTS) {
        record->slot[threadIdx.x].max_packed = 0ull;
        record->slot[threadIdx.x].data_energy = 0.0;
        record->slot[threadIdx.x].smoothing_energy = 0.0;
        record->slot[threadIdx.x].level_set_energy = 0.0;
    }
}

// the most rows ONE iteration of n_lists launches can write on this grid (INTERIOR list or boxes, then BOUNDARY list)
inline int64_t rows_per_iteration_max(const lsf_grid* g, int32_t n_lists) {
    const unsigned list = state_iteration_rows_max(g), boxes = state_iteration_boxes_rows_max(g);
    return (int64_t)(list > boxes ? list : boxes) + (n_lists > 1 ? (int64_t)list : 0);
}

// one timing-less event per host thread and device, created on first use (an event per call costs a create / destroy pair)
inline hipEvent_t thread_event() {
    thread_local hipEvent_t events[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    if (!events[dev] && hipEventCreateWithFlags(&events[dev], hipEventDisableTiming) != hipSuccess) events[dev] = nullptr;
    return events[dev];
}

inline bool run_ok(const lsf_state_run* r) {
    return r && r->live && r->canonical && r->state[0] && r->state[1] && r->state[0] != r->state[1] && r->prepare_scratch &&
           r->totals_device && r->totals_host && r->sparse_reach >= 0 && r->sparse_reach <= 8;
}

// The end of a call on the card: the listed finalize pass and, for ONE copy to the host, the records' used words with the 16
// statistics behind them in words_device.  With statistics the pass's one-block combine kernel gathers them as its tail;
// without, nothing combines and the gather is a launch of its own (zeros for the statistics).
inline int finalize_and_gather_words(const float* final_state, const float* canonical, float* live_out, const lsf_grid* g,
                                     const int32_t* const* listed, const int64_t* listed_counts, int n_listed,
                                     int64_t opposite_count, int64_t first_opposite, float lower_threshold,
                                     double* statistics16, double* finalize_scratch, const lsf_iteration_record* guard_records,
                                     int32_t guard_count, float guard_limit, const lsf_iteration_record* records, int n_slots,
                                     int64_t* words_device, hipStream_t s) {
    if (int e = state_finalize_listed_launch(final_state, canonical, live_out, nullptr, g, listed, listed_counts, n_listed,
                                             opposite_count, first_opposite, lower_threshold, statistics16, finalize_scratch,
                                             nullptr, guard_records, guard_count, guard_limit, statistics16 ? records : nullptr,
                                             statistics16 ? n_slots : 0, statistics16 ? words_device : nullptr, s))
        return e;
    if (statistics16) return 0;
    hipLaunchKernelGGL(records_used_words_kernel, dim3((n_slots * 4 + 16 + kBlock - 1) / kBlock), dim3(kBlock), 0, s,
                       reinterpret_cast<const long long*>(records), (const long long*)nullptr,
                       reinterpret_cast<long long*>(words_device), n_slots, 1);
    return launch_status();
}

}  // namespace

extern "C" int64_t lsf_state_run_rows_elements(const lsf_grid* grid, int32_t iterations, int32_t n_lists) {
    if (check_grid(grid) || iterations < 1 || n_lists < 1 || n_lists > 2) return 0;
    return rows_per_iteration_max(grid, n_lists) * iterations * (int64_t)(sizeof(RecordRow) / sizeof(int64_t));
}

extern "C" int lsf_state_run_begin(const lsf_state_run* run, void* stream) {
    if (!run_ok(run)) return LSF_ERR_BAD_ARGUMENT;
    const lsf_grid* g = &run->grid;
    if (int e = check_grid(g)) return e;
    if (g->z_begin != 0 || g->z_end != g->nz) return LSF_ERR_BAD_ARGUMENT;  // whole volumes
    hipStream_t s = as_stream(stream);
    const bool sparse = run->sparse_reach > 0;
    // the counting pass; it also writes the states unless they are initialised near the band only (below).  With
    // second_state_late the second state is written behind the copy of the list sizes, where it overlaps the host's wait
    float* b_in_pass = (sparse || run->second_state_late) ? nullptr : run->state[1];
    // (without boxes to count the pass's scan writes the fifth total, 0, itself)
    if (int e = state_prepare_launch(run->live, run->canonical, sparse ? nullptr : run->state[0], b_in_pass, g,
                                     run->prepare_scratch, run->totals_device, !run->box_scratch, stream))
        return e;
    // (optional) the boxes of the box walk are counted behind the pass, so that their number comes back with the list sizes
    if (run->box_scratch)
        if (int e = lsf_band_boxes_count(g, run->box_all ? LSF_BAND_ALL : LSF_BAND_INTERIOR, run->prepare_scratch, run->box_scratch,
                                         run->totals_device + 4, stream))
            return e;
    if (hipMemcpyAsync(run->totals_host, run->totals_device, 5 * sizeof(int64_t), hipMemcpyDeviceToHost, s) != hipSuccess)
        return (int)hipGetLastError();
    hipEvent_t sizes = thread_event();
    if (!sizes) return (int)hipGetLastError();
    int status = 0;
    if (hipEventRecord(sizes, s) != hipSuccess) status = (int)hipGetLastError();
    if (!status && sparse)
        status = lsf_state_pack_needed(run->live, run->state[0], run->state[1], g, run->prepare_scratch, run->sparse_reach, 0,
                                       stream);
    else if (!status && run->second_state_late)
        status = lsf_state_pack(run->live, nullptr, run->state[1], nullptr, g, stream);
    if (!status && hipEventSynchronize(sizes) != hipSuccess) status = (int)hipGetLastError();
    return status;
}

extern "C" int lsf_state_run_finish(const lsf_state_run* run, const lsf_slavcheva_params* params, int32_t* list_interior,
                                    int32_t* list_boundary, lsf_band_box* boxes, float* box_canonical,
                                    lsf_iteration_record* records, int32_t iterations, const lsf_run_loop* loop,
                                    float* live_out, float lower_threshold, double* statistics16,
                                    double* finalize_scratch, int64_t* words_device, int64_t* words_host,
                                    lsf_state_run_result* result, void* stream) {
    return lsf_state_run_finish_rows(run, params, list_interior, list_boundary, boxes, box_canonical, records, iterations, loop,
                                     live_out, lower_threshold, statistics16, finalize_scratch, words_device, words_host,
                                     result, nullptr, 0, nullptr, stream);
}

extern "C" int lsf_state_run_finish_rows(const lsf_state_run* run, const lsf_slavcheva_params* params, int32_t* list_interior,
                                         int32_t* list_boundary, lsf_band_box* boxes, float* box_canonical,
                                         lsf_iteration_record* records, int32_t iterations, const lsf_run_loop* loop,
                                         float* live_out, float lower_threshold, double* statistics16,
                                         double* finalize_scratch, int64_t* words_device, int64_t* words_host,
                                         lsf_state_run_result* result, int64_t* record_rows, int64_t record_rows_elements,
                                         int32_t* rows_taken, void* stream) {
    if (rows_taken) *rows_taken = 0;
    if (record_rows && (record_rows_elements <= 0 || (reinterpret_cast<uintptr_t>(record_rows) & 31u) != 0))
        return LSF_ERR_BAD_ARGUMENT;
    if (!run_ok(run) || !params || !records || iterations < 1 || !live_out || !words_device || !words_host || !result ||
        (statistics16 && !finalize_scratch) || !result->max_value || !result->argmax ||
        !result->energies3 || !result->executed)
        return LSF_ERR_BAD_ARGUMENT;
    if (loop && (loop->min_iterations < 1 || loop->check_interval < 1 ||
                 (loop->max_iterations > loop->min_iterations ? loop->max_iterations : loop->min_iterations) != iterations))
        return LSF_ERR_BAD_ARGUMENT;
    if (run->box_all && boxes) return LSF_ERR_BAD_ARGUMENT;  // those are lsf_sobolev_run_finish's boxes
    const lsf_grid* g = &run->grid;
    if (int e = check_grid(g)) return e;
    const int64_t n_interior = run->totals_host[0], n_boundary = run->totals_host[1];
    if (n_interior < 0 || n_boundary < 0 || n_interior > 0x7fffffffll || n_boundary > 0x7fffffffll ||
        (n_interior && !list_interior) || (n_boundary && !list_boundary))
        return LSF_ERR_BAD_ARGUMENT;
    // Record rows: a fixed count reads no record before its end, so its launches leave one row per wave (iteration i's
    // launches one behind the other from row i * rows_per_iteration on) and ONE launch behind the last iteration makes the
    // records.  A batch of gated launches keeps the atomics: the next launch's gate and the host read its records.
    const bool fixed = !loop || loop->min_iterations >= iterations;
    RecordRow* const rows = fixed ? reinterpret_cast<RecordRow*>(record_rows) : nullptr;
    const int64_t rows_capacity = rows ? record_rows_elements / (int64_t)(sizeof(RecordRow) / sizeof(int64_t)) : 0;
    if (rows && record_rows_elements <
                    lsf_state_run_rows_elements(g, iterations, (n_interior ? 1 : 0) + ((n_boundary || !n_interior) ? 1 : 0)))
        return LSF_ERR_BAD_ARGUMENT;  // (before anything is launched)
    hipStream_t s = as_stream(stream);
    // the lists, from the ballots the counting pass kept; an empty list is dropped -- but never both (a launch over an
    // empty BOUNDARY list still contributes the arg-max of an all-zero update)
    const int32_t* lists[2];
    int64_t counts[2];
    int32_t subsets[2];
    int n_lists = 0;
    if (n_interior) {
        if (int e = lsf_band_list_fill_prepared(g, LSF_BAND_INTERIOR, run->prepare_scratch, list_interior, stream)) return e;
        lists[n_lists] = list_interior; counts[n_lists] = n_interior; subsets[n_lists++] = LSF_BAND_INTERIOR;
    }
    if (n_boundary || !n_lists) {
        if (n_boundary)
            if (int e = lsf_band_list_fill_prepared(g, LSF_BAND_BOUNDARY, run->prepare_scratch, list_boundary, stream)) return e;
        // (an empty list is never dereferenced; the pointer only has to be non-NULL to mean "a list walk")
        lists[n_lists] = n_boundary ? list_boundary : reinterpret_cast<const int32_t*>(run->prepare_scratch);
        counts[n_lists] = n_boundary; subsets[n_lists++] = LSF_BAND_BOUNDARY;
    }
    // the INTERIOR voxels box by box when the caller asks for it (same results; DESIGN.md section 5: the walk that pays
    // when the band's states do not fit the Infinity Cache)
    const int64_t n_boxes = boxes && run->box_scratch ? run->totals_host[4] : 0;
    if (n_boxes > 0) {
        if (!box_canonical) return LSF_ERR_BAD_ARGUMENT;
        if (int e = lsf_band_boxes_fill(g, LSF_BAND_INTERIOR, run->prepare_scratch, run->box_scratch, boxes, stream)) return e;
        if (int e = lsf_band_boxes_canonical(run->canonical, g, boxes, n_boxes, box_canonical, stream)) return e;
    }
    const bool sparse = run->sparse_reach > 0;
    const int n_slots = iterations * LSF_RECORD_SLOTS;
    // The iterations: iteration i reads state[i % 2] and writes the other.  A fixed count: all of them ungated, at once.
    // With a stop test that can fire (slavcheva_optimizer2d.py:360-362) iteration i >= min_iterations sits behind the
    // device-side gate on record i - 1, and the host looks at the records every check_interval iterations.
    unsigned rows_per_iteration = 0u;
    int32_t it = 0, n_exec = fixed ? iterations : 0;
    while (it < iterations) {
        const int32_t batch = fixed ? iterations : (loop->check_interval < iterations - it ? loop->check_interval : iterations - it);
        for (int32_t i = it; i < it + batch; ++i) {
            lsf_gate gate_i{records + (i > 0 ? i - 1 : 0), LSF_GATE_SLAVCHEVA, loop ? loop->lower_threshold : 0.0f,
                            loop ? loop->upper_threshold : 0.0f};
            const lsf_gate* gate = (fixed || i < loop->min_iterations) ? nullptr : &gate_i;
            int64_t row = (int64_t)i * rows_per_iteration;  // (rows_per_iteration: known from iteration 0 on)
            for (int k = 0; k < n_lists; ++k) {
                int e;
                unsigned written = 0u;
                const unsigned room = rows ? (unsigned)(rows_capacity - row < 0x7fffffffll ? rows_capacity - row : 0x7fffffffll) : 0u;
                if (n_boxes > 0 && subsets[k] == LSF_BAND_INTERIOR)
                    e = state_iteration_boxes_launch(run->state[i % 2], box_canonical, run->state[(i + 1) % 2], g, params, gate,
                                                     records + i, boxes, n_boxes, rows ? rows + row : nullptr, room, &written,
                                                     stream);
                else
                    e = state_iteration_launch(run->state[i % 2], run->canonical, run->state[(i + 1) % 2], g, params, gate,
                                               records + i, lists[k], counts[k], subsets[k], rows ? rows + row : nullptr, room,
                                               &written, stream);
                if (e) return e;
                row += written;
            }
            // every iteration launches the same grids: its rows are as many as iteration 0's
            if (i == 0) rows_per_iteration = (unsigned)row;
            else if (rows && row != (int64_t)(i + 1) * rows_per_iteration) return LSF_ERR_BAD_ARGUMENT;
        }
        it += batch;
        if (rows) {
            if (rows_per_iteration == 0u) return LSF_ERR_BAD_ARGUMENT;  // (a launch always has a workgroup)
            hipLaunchKernelGGL(records_from_rows_kernel, dim3((unsigned)iterations), dim3(kBlock), 0, s, rows, rows_per_iteration,
                               records);
            if (int e = launch_status()) return e;
        }
        if (fixed) break;
        // the batch's records (their used words) to the host, one wait; then the reference's loop condition
        const int first_slot = (it - batch) * LSF_RECORD_SLOTS, batch_slots = batch * LSF_RECORD_SLOTS;
        hipLaunchKernelGGL(records_used_words_kernel, dim3((batch_slots * 4 + kBlock - 1) / kBlock), dim3(kBlock), 0, s,
                           reinterpret_cast<const long long*>(records + (it - batch)), nullptr,
                           reinterpret_cast<long long*>(words_device) + (size_t)first_slot * 4, batch_slots, 0);
        if (int e = launch_status()) return e;
        if (hipMemcpyAsync(words_host + (size_t)first_slot * 4, words_device + (size_t)first_slot * 4,
                           (size_t)batch_slots * 4 * sizeof(int64_t), hipMemcpyDeviceToHost, s) != hipSuccess)
            return (int)hipGetLastError();
        if (hipStreamSynchronize(s) != hipSuccess) return (int)hipGetLastError();
        if (int e = lsf_records_decode(words_host, it, LSF_RECORD_SLOTS, 4, result->max_value, result->argmax,
                                       result->energies3, result->executed))
            return e;
        n_exec = 0;
        while (n_exec < it && result->executed[n_exec]) ++n_exec;
        if (n_exec < it) break;  // the gate closed inside the batch
        const float m = result->max_value[n_exec - 1];
        if (n_exec >= loop->min_iterations && !(loop->lower_threshold < m && m < loop->upper_threshold)) break;
    }
    // the end of the call behind the last iteration: the listed voxels' live values into the caller's array (which holds
    // the input everywhere else) and the convergence statistics; with sparsely initialised states the pass looks at the
    // records first and leaves everything alone when an update outran what was initialised
    const float* final_state = run->state[n_exec % 2];
    int64_t listed_counts[2] = {0, 0};
    const int32_t* listed[2] = {nullptr, nullptr};
    int n_listed = 0;
    for (int k = 0; k < n_lists; ++k)
        if (counts[k]) { listed[n_listed] = lists[k]; listed_counts[n_listed++] = counts[k]; }
    if (int e = finalize_and_gather_words(final_state, run->canonical, live_out, g, listed, listed_counts, n_listed,
                                          run->totals_host[2], run->totals_host[3], lower_threshold, statistics16,
                                          finalize_scratch, sparse ? records : nullptr, sparse ? iterations : 0,
                                          (float)run->sparse_reach, records, n_slots, words_device, s))
        return e;
    if (hipMemcpyAsync(words_host, words_device, ((size_t)n_slots * 4 + 16) * sizeof(int64_t), hipMemcpyDeviceToHost, s) !=
        hipSuccess)
        return (int)hipGetLastError();
    if (hipStreamSynchronize(s) != hipSuccess) return (int)hipGetLastError();
    if (int e = lsf_records_decode(words_host, iterations, LSF_RECORD_SLOTS, 4, result->max_value, result->argmax,
                                   result->energies3, result->executed))
        return e;
    result->final_state = n_exec % 2;
    result->n_lists = n_lists;
    result->reach_exceeded = 0;
    result->compact_faces = -1;
    if (rows_taken) *rows_taken = rows ? 1 : 0;
    for (int32_t i = 0; i < iterations && sparse; ++i)
        if (result->executed[i] && !(result->max_value[i] < (float)run->sparse_reach)) result->reach_exceeded = 1;
    return 0;
}

// the same call with the SobolevFusion iteration (gradient + x pass over the list of all band voxels, then y pass, z pass,
// update and re-warp box by box): engine_run._optimize_run(sobolev=True)
extern "C" int lsf_sobolev_run_finish(const lsf_state_run* run, const lsf_slavcheva_params* params, const double* taps_host,
                                      int32_t n_taps, int32_t* list_interior, int32_t* list_boundary, int32_t* list_all,
                                      lsf_band_box* boxes, float* g4_a, float* g4_b, lsf_iteration_record* records,
                                      int32_t iterations, const lsf_run_loop* loop, float* live_out, float lower_threshold,
                                      double* statistics16, double* finalize_scratch, int64_t* words_device,
                                      int64_t* words_host, lsf_state_run_result* result, void* stream) {
    if (!run_ok(run) || !run->box_scratch || !run->box_all || !params || !taps_host || !boxes || !g4_a || !g4_b ||
        g4_a == g4_b || !records || iterations < 1 || !live_out || !words_device || !words_host || !result ||
        (statistics16 && !finalize_scratch) || !result->max_value || !result->argmax || !result->energies3 ||
        !result->executed)
        return LSF_ERR_BAD_ARGUMENT;
    if (loop && (loop->min_iterations < 1 || loop->check_interval < 1 ||
                 (loop->max_iterations > loop->min_iterations ? loop->max_iterations : loop->min_iterations) != iterations))
        return LSF_ERR_BAD_ARGUMENT;
    const lsf_grid* g = &run->grid;
    if (int e = check_grid(g)) return e;
    if (g->dims != 3) return LSF_ERR_BAD_DIMS;
    const int64_t n_interior = run->totals_host[0], n_boundary = run->totals_host[1], n_boxes = run->totals_host[4];
    if (n_interior < 0 || n_boundary < 0 || n_boxes < 0 || n_interior + n_boundary > 0x7fffffffll ||
        (n_interior && !list_interior) || (n_boundary && !list_boundary) || (n_interior && n_boundary && !list_all))
        return LSF_ERR_BAD_ARGUMENT;
    hipStream_t s = as_stream(stream);
    if (n_interior)
        if (int e = lsf_band_list_fill_prepared(g, LSF_BAND_INTERIOR, run->prepare_scratch, list_interior, stream)) return e;
    if (n_boundary)
        if (int e = lsf_band_list_fill_prepared(g, LSF_BAND_BOUNDARY, run->prepare_scratch, list_boundary, stream)) return e;
    // ONE ascending list of the whole band for the fused gradient + x pass (a tap at a voxel of another list would count as zero)
    const int32_t* all = n_interior ? list_interior : list_boundary;
    const int64_t n_all = n_interior + n_boundary;
    if (n_interior && n_boundary) {
        const int32_t* a[1] = {list_interior};
        const int32_t* b[1] = {list_boundary};
        int32_t* out[1] = {list_all};
        const int64_t na[1] = {n_interior}, nb[1] = {n_boundary};
        if (int e = lsf_merge_sorted_runs(a, na, b, nb, out, 1, stream)) return e;
        all = list_all;
    }
    if (n_boxes > 0)
        if (int e = lsf_band_boxes_fill(g, LSF_BAND_ALL, run->prepare_scratch, run->box_scratch, boxes, stream)) return e;
    const bool sparse = run->sparse_reach > 0;
    const int n_slots = iterations * LSF_RECORD_SLOTS;
    const bool fixed = !loop || loop->min_iterations >= iterations;
    int32_t it = 0, n_exec = fixed ? iterations : 0;
    while (it < iterations) {
        const int32_t batch = fixed ? iterations : (loop->check_interval < iterations - it ? loop->check_interval : iterations - it);
        for (int32_t i = it; i < it + batch; ++i) {
            lsf_gate gate_i{records + (i > 0 ? i - 1 : 0), LSF_GATE_SLAVCHEVA, loop ? loop->lower_threshold : 0.0f,
                            loop ? loop->upper_threshold : 0.0f};
            const lsf_gate* gate = (fixed || i < loop->min_iterations) ? nullptr : &gate_i;
            const float* s_in = run->state[i % 2];
            float* s_out = run->state[(i + 1) % 2];
            if (n_all)
                if (int e = lsf_sobolev_state_gradient_x(s_in, run->canonical, g4_a, g, params, taps_host, n_taps, gate,
                                                         records + i, all, n_all, 1, stream))
                    return e;
            // the filtered gradient is an OUTPUT of the last executed iteration only: a fixed count stores just that one
            float* g_out = (!fixed || i == iterations - 1) ? g4_b : nullptr;
            if (int e = lsf_sobolev_state_update_boxes(g4_a, s_in, s_out, g_out, g, params, taps_host, n_taps, gate, records + i,
                                                       boxes, n_boxes, stream))
                return e;
        }
        it += batch;
        if (fixed) break;
        const int first_slot = (it - batch) * LSF_RECORD_SLOTS, batch_slots = batch * LSF_RECORD_SLOTS;
        hipLaunchKernelGGL(records_used_words_kernel, dim3((batch_slots * 4 + kBlock - 1) / kBlock), dim3(kBlock), 0, s,
                           reinterpret_cast<const long long*>(records + (it - batch)), nullptr,
                           reinterpret_cast<long long*>(words_device) + (size_t)first_slot * 4, batch_slots, 0);
        if (int e = launch_status()) return e;
        if (hipMemcpyAsync(words_host + (size_t)first_slot * 4, words_device + (size_t)first_slot * 4,
                           (size_t)batch_slots * 4 * sizeof(int64_t), hipMemcpyDeviceToHost, s) != hipSuccess)
            return (int)hipGetLastError();
        if (hipStreamSynchronize(s) != hipSuccess) return (int)hipGetLastError();
        if (int e = lsf_records_decode(words_host, it, LSF_RECORD_SLOTS, 4, result->max_value, result->argmax,
                                       result->energies3, result->executed))
            return e;
        n_exec = 0;
        while (n_exec < it && result->executed[n_exec]) ++n_exec;
        if (n_exec < it) break;
        const float m = result->max_value[n_exec - 1];
        if (n_exec >= loop->min_iterations && !(loop->lower_threshold < m && m < loop->upper_threshold)) break;
    }
    const int32_t* listed[2] = {nullptr, nullptr};
    int64_t listed_counts[2] = {0, 0};
    int n_listed = 0;
    if (n_interior) { listed[n_listed] = list_interior; listed_counts[n_listed++] = n_interior; }
    if (n_boundary) { listed[n_listed] = list_boundary; listed_counts[n_listed++] = n_boundary; }
    if (int e = finalize_and_gather_words(run->state[n_exec % 2], run->canonical, live_out, g, listed, listed_counts, n_listed,
                                          run->totals_host[2], run->totals_host[3], lower_threshold, statistics16,
                                          finalize_scratch, sparse ? records : nullptr, sparse ? iterations : 0,
                                          (float)run->sparse_reach, records, n_slots, words_device, s))
        return e;
    if (hipMemcpyAsync(words_host, words_device, ((size_t)n_slots * 4 + 16) * sizeof(int64_t), hipMemcpyDeviceToHost, s) !=
        hipSuccess)
        return (int)hipGetLastError();
    if (hipStreamSynchronize(s) != hipSuccess) return (int)hipGetLastError();
    if (int e = lsf_records_decode(words_host, iterations, LSF_RECORD_SLOTS, 4, result->max_value, result->argmax,
                                   result->energies3, result->executed))
        return e;
    result->final_state = n_exec % 2;
    result->n_lists = n_listed;
    result->reach_exceeded = 0;
    result->compact_faces = -1;
    for (int32_t i = 0; i < iterations && sparse; ++i)
        if (result->executed[i] && !(result->max_value[i] < (float)run->sparse_reach)) result->reach_exceeded = 1;
    return 0;
}
