// Placement plans (gfx950): the strided copies of combine_legs / split_legs for a block structure that comes back.
//
// cyb_copy_strided_batched receives one descriptor with two ADDRESSES per copy and normalises, classifies, cuts and
// uploads the whole list in every call.  A plan does that once: its records name their blocks by row of two address
// tables, the normalised records and the work items stay in device memory, and an enqueue uploads the two tables only.
// The kernels are the bodies of copy_kernels.h behind one table lookup per work item.
#include "common.h"
#include "copy_kernels.h"

namespace {

using namespace cyb_copy;
using namespace cyb_flat; // Item, NT, chunk_real, cut

// device records: the normalised copy (its own address fields unused) + where the two blocks are found
struct PlaceRow {
    CopyDev d;
    int32_t rblock, wblock; // rows of the table that is read / written
    int64_t roff, woff;     // element offsets inside the two blocks
};
struct PlaceTile {
    CopyT d;
    int32_t rblock, wblock;
    int64_t roff, woff;
};

template <typename T>
__global__ void __launch_bounds__(NT) place_strided_kernel(const PlaceRow* __restrict__ recs, const Item* __restrict__ items,
                                                           const int64_t* __restrict__ rtab, const int64_t* __restrict__ wtab)
{
    const Item it = items[blockIdx.x];
    const PlaceRow r = recs[it.desc];
    copy_strided_body<T>(r.d, (const GLOBAL_AS T*)rtab[r.rblock] + r.roff, (GLOBAL_AS T*)wtab[r.wblock] + r.woff, it);
}

template <typename T>
__global__ void __launch_bounds__(NT) place_transpose_kernel(const PlaceTile* __restrict__ recs, const Item* __restrict__ items,
                                                             const int64_t* __restrict__ rtab, const int64_t* __restrict__ wtab)
{
    __shared__ T tile[32][33];
    const Item it = items[blockIdx.x];
    const PlaceTile r = recs[it.desc];
    copy_transpose_body<T>(r.d, (const GLOBAL_AS T*)rtab[r.rblock] + r.roff, (GLOBAL_AS T*)wtab[r.wblock] + r.woff, it, tile);
}

__global__ void __launch_bounds__(NT) place_transpose64_kernel(const PlaceTile* __restrict__ recs, const Item* __restrict__ items,
                                                               const int64_t* __restrict__ rtab, const int64_t* __restrict__ wtab)
{
    __shared__ __attribute__((aligned(16))) double tile[T64_TS * T64_LS];
    const Item it = items[blockIdx.x];
    const PlaceTile r = recs[it.desc];
    copy_transpose64_body(r.d, (gcp)rtab[r.rblock] + r.roff, (gp)wtab[r.wblock] + r.woff, it, tile);
}

// one direction of a plan, resident on the device
struct Direction {
    bool built = false;
    void* blob = nullptr;
    const PlaceRow* rows = nullptr;
    const Item* items = nullptr;
    const PlaceTile* tiles = nullptr;
    const Item* titems = nullptr;
    int64_t n_items = 0, n_titems = 0;
};

} // namespace

struct cyb_place_plan_s {
    int device = 0;
    int32_t elem_size = 8;
    int64_t n_src = 0, n_dst = 0;
    std::vector<cyb_place_rec> recs;       // the non-empty records as given
    std::vector<char> src_used, dst_used;  // blocks a non-empty record names: their address must not be 0
    Direction dir[2];                      // [0] src -> dst, [1] dst -> src
};

namespace {

// Normalise, classify and cut the records for one direction and copy the result to the device (synchronous).
int build_direction(cyb_place_plan_s* pl, int reverse)
{
    Direction& D = pl->dir[reverse];
    std::vector<PlaceRow> rows;
    std::vector<PlaceTile> tiles;
    std::vector<Item> items, titems;
    std::vector<int64_t> totals, tile_totals; // elements of a row, tiles of a tiled record
    const int64_t tsz = pl->elem_size == 8 ? 64 : 32;
    for (const cyb_place_rec& r : pl->recs) {
        const int64_t* rs = reverse ? r.dst_strides : r.src_strides; // strides on the side that is read
        const int64_t* ws = reverse ? r.src_strides : r.dst_strides;
        PlaceRow row;
        memset(&row, 0, sizeof(row));
        normalize_copy(r.shape, ws, rs, r.ndim, row.d); // (extents were checked at creation)
        row.rblock = reverse ? r.dst_block : r.src_block;
        row.wblock = reverse ? r.src_block : r.dst_block;
        row.roff = reverse ? r.dst_offset : r.src_offset;
        row.woff = reverse ? r.src_offset : r.dst_offset;
        PlaceTile t;
        int64_t ntile = 0;
        if (classify_transpose(row.d, tsz, t.d, ntile)) {
            t.rblock = row.rblock, t.wblock = row.wblock, t.roff = row.roff, t.woff = row.woff;
            tiles.push_back(t);
            tile_totals.push_back(ntile);
            continue;
        }
        rows.push_back(row);
        totals.push_back(row.d.total);
    }
    CYB_REQUIRE(cut(titems, tile_totals, tiles_per_item(tsz)) && cut(items, totals, chunk_real(sum_of(totals))),
                "cyb_place_plan: too many work items");
    // one allocation, each part 256-byte aligned
    const size_t parts[4] = {sizeof(PlaceRow) * rows.size(), sizeof(Item) * items.size(), sizeof(PlaceTile) * tiles.size(),
                             sizeof(Item) * titems.size()};
    const void* srcs[4] = {rows.data(), items.data(), tiles.data(), titems.data()};
    size_t off[4], tot = 0;
    for (int k = 0; k < 4; ++k) {
        off[k] = tot;
        tot += (parts[k] + 255) / 256 * 256;
    }
    if (tot) {
        std::vector<char> img(tot, 0);
        for (int k = 0; k < 4; ++k)
            if (parts[k]) memcpy(img.data() + off[k], srcs[k], parts[k]);
        hipError_t e = hipMalloc(&D.blob, tot);
        if (e != hipSuccess) {
            D.blob = nullptr;
            cyb::set_error("cyb_place_plan: hipMalloc(%zu) failed: %s", tot, hipGetErrorString(e));
            return CYB_ERR_NOMEM;
        }
        e = hipMemcpy(D.blob, img.data(), tot, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(D.blob);
            D.blob = nullptr;
            cyb::set_error("cyb_place_plan: hipMemcpy failed: %s", hipGetErrorString(e));
            return CYB_ERR_HIP;
        }
        char* b = static_cast<char*>(D.blob);
        D.rows = reinterpret_cast<const PlaceRow*>(b + off[0]);
        D.items = reinterpret_cast<const Item*>(b + off[1]);
        D.tiles = reinterpret_cast<const PlaceTile*>(b + off[2]);
        D.titems = reinterpret_cast<const Item*>(b + off[3]);
    }
    D.n_items = (int64_t)items.size();
    D.n_titems = (int64_t)titems.size();
    D.built = true;
    return CYB_OK;
}

} // namespace

extern "C" {

int cyb_place_plan_create(cyb_ctx_t ctx, const cyb_place_rec* recs, int64_t n, int64_t n_src, int64_t n_dst, int32_t elem_size,
                          cyb_place_plan_t* out)
{
    CYB_REQUIRE(ctx && out, "cyb_place_plan_create: NULL argument");
    CYB_REQUIRE(n >= 0 && (n == 0 || recs), "cyb_place_plan_create: bad record list");
    CYB_REQUIRE(n_src >= 0 && n_dst >= 0 && n_src <= INT32_MAX && n_dst <= INT32_MAX, "cyb_place_plan_create: bad table sizes");
    CYB_REQUIRE(elem_size == 8 || elem_size == 16, "cyb_place_plan_create: unsupported elem_size %d", elem_size);
    std::vector<cyb_place_rec> kept;
    std::vector<char> src_used((size_t)n_src, 0), dst_used((size_t)n_dst, 0);
    for (int64_t i = 0; i < n; ++i) {
        const cyb_place_rec& r = recs[i];
        CYB_REQUIRE(r.ndim >= 0 && r.ndim <= CYB_MAX_NDIM, "place rec %lld: ndim %d out of range", (long long)i, r.ndim);
        CYB_REQUIRE(r.src_block >= 0 && r.src_block < n_src, "place rec %lld: src_block %d outside the table of %lld", (long long)i,
                    r.src_block, (long long)n_src);
        CYB_REQUIRE(r.dst_block >= 0 && r.dst_block < n_dst, "place rec %lld: dst_block %d outside the table of %lld", (long long)i,
                    r.dst_block, (long long)n_dst);
        CYB_REQUIRE(r.src_offset >= 0 && r.dst_offset >= 0, "place rec %lld: negative offset", (long long)i);
        int64_t tot = 1;
        for (int k = 0; k < r.ndim; ++k) {
            CYB_REQUIRE(r.shape[k] >= 0, "place rec %lld: negative extent", (long long)i);
            tot *= r.shape[k];
        }
        if (tot == 0) continue;
        src_used[(size_t)r.src_block] = dst_used[(size_t)r.dst_block] = 1;
        kept.push_back(r);
    }
    cyb_place_plan_s* pl = new cyb_place_plan_s();
    pl->device = ctx->device;
    pl->elem_size = elem_size;
    pl->n_src = n_src;
    pl->n_dst = n_dst;
    pl->recs.swap(kept);
    pl->src_used.swap(src_used);
    pl->dst_used.swap(dst_used);
    const int rc = build_direction(pl, 0);
    if (rc != CYB_OK) {
        delete pl;
        return rc;
    }
    *out = pl;
    return CYB_OK;
}

int cyb_place_plan_enqueue(cyb_ctx_t ctx, cyb_place_plan_t pl, const int64_t* src_ptrs, const int64_t* dst_ptrs, int32_t reverse)
{
    CYB_REQUIRE(ctx && pl, "cyb_place_plan_enqueue: NULL argument");
    CYB_REQUIRE(reverse == 0 || reverse == 1, "cyb_place_plan_enqueue: reverse must be 0 or 1");
    CYB_REQUIRE(ctx->device == pl->device, "cyb_place_plan_enqueue: the plan was made on another device");
    if (pl->recs.empty()) return CYB_OK;
    CYB_REQUIRE(src_ptrs && dst_ptrs, "cyb_place_plan_enqueue: NULL address table");
    for (int64_t i = 0; i < pl->n_src; ++i)
        CYB_REQUIRE(src_ptrs[i] != 0 || !pl->src_used[(size_t)i], "cyb_place_plan_enqueue: src block %lld has no address", (long long)i);
    for (int64_t i = 0; i < pl->n_dst; ++i)
        CYB_REQUIRE(dst_ptrs[i] != 0 || !pl->dst_used[(size_t)i], "cyb_place_plan_enqueue: dst block %lld has no address", (long long)i);
    Direction& D = pl->dir[reverse];
    if (!D.built) CYB_TRY(build_direction(pl, reverse));
    void *d_src = nullptr, *d_dst = nullptr;
    CYB_TRY(cyb::upload_packed(ctx, {{src_ptrs, sizeof(int64_t) * (size_t)pl->n_src, &d_src}, {dst_ptrs, sizeof(int64_t) * (size_t)pl->n_dst, &d_dst}}));
    const int64_t* rtab = static_cast<const int64_t*>(reverse ? d_dst : d_src);
    const int64_t* wtab = static_cast<const int64_t*>(reverse ? d_src : d_dst);
    const dim3 block(NT);
    if (D.n_titems) {
        const dim3 grid((unsigned)D.n_titems);
        if (pl->elem_size == 8) hipLaunchKernelGGL(place_transpose64_kernel, grid, block, 0, ctx->stream, D.tiles, D.titems, rtab, wtab);
        else hipLaunchKernelGGL(place_transpose_kernel<u128>, grid, block, 0, ctx->stream, D.tiles, D.titems, rtab, wtab);
        CYB_HIP(hipGetLastError());
    }
    if (D.n_items) {
        const dim3 grid((unsigned)D.n_items);
        if (pl->elem_size == 8) hipLaunchKernelGGL(place_strided_kernel<uint64_t>, grid, block, 0, ctx->stream, D.rows, D.items, rtab, wtab);
        else hipLaunchKernelGGL(place_strided_kernel<u128>, grid, block, 0, ctx->stream, D.rows, D.items, rtab, wtab);
        CYB_HIP(hipGetLastError());
    }
    return CYB_OK;
}

int cyb_place_plan_destroy(cyb_place_plan_t pl)
{
    if (!pl) return CYB_OK;
    if (pl->dir[0].blob || pl->dir[1].blob) {
        (void)hipDeviceSynchronize(); // an enqueued kernel may still read the plan
        for (Direction& D : pl->dir)
            if (D.blob) (void)hipFree(D.blob);
    }
    delete pl;
    return CYB_OK;
}

} // extern "C"
