"""Puts two tools/pmc_summary.py summaries -- the parent commit's and this build's, taken in one visit -- into one file, with
the dense SpMM launch's derived figures: the reads that are not gathers (TCC_REQ - stores - nnz * tiles * 2) and the fetch
that is not gathers (with no gather hit in L2, and at an assumed gather hit rate).

    python tools/pmc_before_after.py <before_summary.json> <after_summary.json> <n> <nnz> <tiles> <out.json> [<extra.json>]

extra.json (optional): a further summary kept under "variant" (TCC counters of its SpMM kernels only)."""
import json
import sys

GATHER_HIT = 0.075   # what an XCD's 16 K-row L2 share gives on C4's skew (7-8 %)


def derived(e, n, nnz, tiles, G):
    gather_req = nnz * tiles * 2
    write_req = e["WRITE_SIZE_per_launch"] * 1024 / 128
    fetch = 2 * e["FETCH_SIZE_per_launch"] * 1024
    gather_bytes = nnz * tiles * G * 8
    return {"TCC_REQ": e["TCC_REQ_sum_per_launch"], "TCC_HIT": e["TCC_HIT_sum_per_launch"], "TCC_MISS": e["TCC_MISS_sum_per_launch"],
            "fetch_bytes_FETCH_SIZE_x2": fetch, "write_bytes": e["WRITE_SIZE_per_launch"] * 1024,
            "gather_requests_nnz_x_tiles_x_2": gather_req, "write_requests_128B": write_req,
            "non_gather_read_requests": e["TCC_REQ_sum_per_launch"] - write_req - gather_req,
            "non_gather_fetch_bytes_if_no_gather_hits": fetch - gather_bytes,
            f"non_gather_fetch_bytes_at_{GATHER_HIT:.3f}_gather_hits": fetch - gather_bytes * (1 - GATHER_HIT)}


def main():
    before, after = json.load(open(sys.argv[1])), json.load(open(sys.argv[2]))
    n, nnz, tiles = int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    dense = "rwr::k_spmm_chunked<32, 16, false, false, true, false>"
    out = {"config": after["config"], "correction": after["correction"], "graph": {"n": n, "nnz": nnz, "tiles": tiles},
           "dense_launch_derived": {"kernel": dense, "before": derived(before["kernels"][dense], n, nnz, tiles, 32),
                                    "after": derived(after["kernels"][dense], n, nnz, tiles, 32)},
           "before": before["kernels"], "after": after["kernels"]}
    if len(sys.argv) > 7:
        v = json.load(open(sys.argv[7]))
        out["variant"] = {"config": v["config"],
                          "kernels": {k: {c: x for c, x in e.items() if "TCC" in c or c == "l2_hit_rate"}
                                      for k, e in v["kernels"].items() if "k_spmm" in k}}
    json.dump(out, open(sys.argv[6], "w"), indent=1)
    print(json.dumps(out["dense_launch_derived"], indent=1))


if __name__ == "__main__":
    main()
