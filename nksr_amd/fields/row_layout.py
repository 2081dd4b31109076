"""Where every site's rows start in the ONE Morton-ordered row list of the matrix-free operator (integer arithmetic only: pure
torch, no call into the library, any device -- the CPU tests run it; the product passes GPU tensors).

The list is the stable merge of the site sets by level-0 Morton key (set 0 first on equal keys); a site owns
``rows_per_site`` consecutive rows.  With segments (the chunks of a batched solve) every segment's rows start on a workgroup
boundary of the sweep (256 rows): which cells meet in a workgroup, the partial blocks of the others -- and with them every
summation order of the operator -- are then the same whether the segment is solved alone or with others."""
import torch

SEGMENT_ALIGN = 256     # rows of one workgroup of the sweep
ITEM_ROWS = 32          # rows of one work item


def first_rows_from_ranks(n_a, n_b, rank_a, rank_b, rows_a, rows_b):
    """First rows of two sorted site sets in their merged list: a site's own sites before it + the other set's sites before it.
    ``rank_a[i]``: sites of set b with a SMALLER key than site i of set a; ``rank_b[j]``: sites of set a with a smaller OR EQUAL key."""
    fa = torch.arange(n_a, dtype=torch.int32, device=rank_a.device) * rows_a + rank_a * rows_b
    fb = torch.arange(n_b, dtype=torch.int32, device=rank_b.device) * rows_b + rank_b * rows_a
    return fa, fb


def pad_segments(first_rows, keys, rows_per_site, segments):
    """Move every segment's rows to the next multiple of 256.  ``first_rows`` / ``keys`` / ``rows_per_site``: per site set (one or
    two) the unpadded first rows, the sorted level-0 keys and the rows a site owns; ``segments``: key_lo, nseg, of_keys().
    Returns (padded first rows per set, rows_total, pad_rows, item_seg): pad rows have no site (row_cells = -1, zero values);
    item_seg names the segment of every 32-row work item (the solve skips the items of converged segments)."""
    klo = segments.key_lo
    dev = klo.device
    rows_total = sum(int(k.numel()) * c for k, c in zip(keys, rows_per_site))
    rb = sum(torch.searchsorted(k, klo) * c for k, c in zip(keys, rows_per_site)).long()
    rb = torch.cat([rb, rb.new_tensor([rows_total])])                              # unpadded row bounds [nseg + 1]
    pad = (rb[:-1] - rb[1:]) % SEGMENT_ALIGN
    pad_before = torch.cumsum(pad, 0) - pad
    pb32 = pad_before.to(torch.int32)
    first_rows = [f + pb32[segments.of_keys(k)] for f, k in zip(first_rows, keys)]
    ends = rb[1:] + pad_before                                                     # first pad row of every segment
    ar = torch.arange(SEGMENT_ALIGN - 1, device=dev)[None]
    pad_rows = (ends[:, None] + ar)[ar < pad[:, None]]
    rows_total += int(pad.sum().item())
    item_start = (rb[:-1] + pad_before) // ITEM_ROWS
    item_seg = torch.bucketize(torch.arange(rows_total // ITEM_ROWS + 2, device=dev), item_start, right=True) - 1
    return first_rows, rows_total, pad_rows, item_seg.clamp_(0, segments.nseg - 1).to(torch.int32)
