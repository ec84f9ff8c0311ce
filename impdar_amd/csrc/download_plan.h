// The host-side plan of a staged device -> host download (download.hip): how the blocks of a call are cut into pieces,
// and where each piece lies in the staging ring -- plain C++, no HIP include, compiled by itself in
// tests/test_download_plan.py.  download.hip decides neither.
//
// A block is `count` elements that may only be cut between granules of `gran` elements: the row width of a block of
// rows, 16 for a flat array (whose last granule may be short).  A block of B bytes becomes max(1, ceil(B / (cap / 4)))
// near-equal pieces -- four copies in flight round a ring of `cap` bytes -- but never more pieces than granules.  A
// piece of several granules is then below cap / 2 and a piece of one granule is that granule: a granule above `cap`
// is the only thing that does not fit.
#pragma once
#include <cstddef>
#include <vector>

enum { DL_OK = 0, DL_ERR_GRANULE = 1 };

struct DlBlock {
    size_t count, gran;             // elements, elements per granule (>= 1)
};
struct DlPiece {
    int block;
    size_t first, count, bytes;     // first element within the block, elements, count * elem
};

// the pieces of every block, in block order and in element order within a block; an empty block has none
static inline int download_plan(size_t cap, size_t elem, const DlBlock *blk, int nblk, std::vector<DlPiece> &pieces)
{
    pieces.clear();
    const size_t quarter = cap / 4 ? cap / 4 : 1;
    for (int i = 0; i < nblk; ++i) {
        const size_t n = blk[i].count, gran = blk[i].gran;
        if (n == 0) continue;
        if ((n < gran ? n : gran) * elem > cap) return DL_ERR_GRANULE;
        const size_t granules = (n + gran - 1) / gran, want = (n * elem + quarter - 1) / quarter;
        const size_t np = want < granules ? want : granules;
        for (size_t c = 0; c < np; ++c) {
            const size_t a = granules * c / np * gran, b = c + 1 == np ? n : granules * (c + 1) / np * gran;
            pieces.push_back(DlPiece{i, a, b - a, (b - a) * elem});
        }
    }
    return DL_OK;
}

// Where the pieces lie in a ring of `cap` bytes.  They are placed in order and retired in order, so what is live is one
// interval [tail, head) -- or, once the head has gone round, [tail, wrap_end) and [0, head).  A piece is never split:
// one that does not fit behind the head starts again at 0 and leaves [wrap_end, cap) unused until the tail has passed it.
struct DlRing {
    size_t cap, head = 0, tail = 0, wrap_end = 0, live = 0;
    bool wrapped = false;
    explicit DlRing(size_t c) : cap(c) {}
    // false: retire the oldest live piece first (with none live, any piece of at most `cap` bytes is placed)
    bool place(size_t bytes, size_t *off)
    {
        if (live == 0) {
            head = tail = 0;
            wrapped = false;
        }
        if (wrapped ? head + bytes > tail : head + bytes > cap) {
            if (wrapped || bytes > tail) return false;
            wrap_end = head;
            wrapped = true;
            head = 0;
        }
        *off = head;
        head += bytes;
        ++live;
        return true;
    }
    // the oldest live piece, of `bytes`, has been copied out
    void retire(size_t bytes)
    {
        tail += bytes;
        --live;
        if (wrapped && tail == wrap_end) {
            tail = 0;
            wrapped = false;
        }
    }
};

#ifdef DOWNLOAD_PLAN_PROBE
// What tests/test_download_plan.py calls.  The pieces of the blocks (count[i], gran[i]) as rows {block, first, count,
// bytes, offset, retired} of `out`: where the replay "place, else retire the oldest and try again" put the piece, and
// how many pieces it had retired by then (pieces retired ... k are live once k is placed).  Returns the number of
// pieces, -1 for DL_ERR_GRANULE, -2 when `out` is too short, -3 when the replay found nothing left to retire.
extern "C" long long impdar_download_plan_probe(size_t cap, size_t elem, int nblk, const size_t *count, const size_t *gran,
                                                long long *out, long long max_pieces)
{
    std::vector<DlBlock> blk;
    for (int i = 0; i < nblk; ++i) blk.push_back(DlBlock{count[i], gran[i]});
    std::vector<DlPiece> pieces;
    if (download_plan(cap, elem, blk.data(), nblk, pieces) != DL_OK) return -1;
    if ((long long)pieces.size() > max_pieces) return -2;
    DlRing ring(cap);
    size_t oldest = 0;
    for (size_t k = 0; k < pieces.size(); ++k) {
        size_t off = 0;
        while (!ring.place(pieces[k].bytes, &off)) {
            if (oldest >= k) return -3;
            ring.retire(pieces[oldest++].bytes);
        }
        const DlPiece &q = pieces[k];
        const long long row[6] = {q.block, (long long)q.first, (long long)q.count, (long long)q.bytes, (long long)off, (long long)oldest};
        for (int j = 0; j < 6; ++j) out[6 * k + j] = row[j];
    }
    return (long long)pieces.size();
}
#endif
