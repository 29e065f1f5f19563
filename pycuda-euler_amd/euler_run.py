"""euler_run -- command-line assembler: read file -> contigs (FASTA) and GFA, on 1..8 GPUs.

Replaces the reference's distribution front-end, Spark mapPartitions(assemble2) over read
partitions (src/cli_spark_gpu.py:37), whose per-partition contigs were never merged (SURVEY
§8f row 3), with one process per GPU and a correct global result:

    python pycuda-euler_amd/euler_run.py -i reads.fa -k 31 -o contigs.fa --gfa graph.gfa
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 pycuda-euler_amd/euler_run.py -i reads.fq -k 31 ...

Every rank parses the file with the native reader (csrc/ingest.cpp) and moves only its
contiguous read shard to its GPU; the counts are exchanged by owner with one RCCL
all-to-all-v, owners merge and filter, and the graph is built, ranked and emitted in owner
segments (distributed.sharded_assemble: junction join, partitioned finish).  Rank 0 writes
the outputs.  With one process the fused single-GPU path runs instead (--sharded: the sharded
path at any world size).  --backend gloo with --device N puts every rank on GPU N, the
collectives staged through host memory (tests: several ranks of the real engine on one GPU).
Contigs equal referenceAssembler.all_contigs(build(reads, k, limit), k) with reads parsed as
--fasta-mode says.  --clip-tips (one process, fused path) goes beyond the reference: tips are
clipped on the device (eulerhip.Session.clip_tips; --tip-len, --tip-rounds) before the outputs
are written, and the ClipInfo line goes to stderr.  --pop-bubbles (same path) pops bubbles
(eulerhip.Session.pop_bubbles; --bubble-len, --bubble-rounds), after the tips if both are given,
and the PopInfo line goes to stderr.  --auto-limit (same path) reads the solid limit off the
assembly's k-mer count spectrum (eulerhip.spectrum_threshold; --spectrum-bins) and re-filters the
dict by it on the device, before the tips and bubbles; the chosen limit, or that none was found,
goes to stderr, and --spectrum-out FILE gets the spectrum's non-zero bins as count<TAB>k-mers.
--limit auto is the form of it that works on every path: on the fused path it is --limit 1
--auto-limit; with --sharded or several ranks the owner merge runs at limit 1, the ranks' spectra
of their owner segments are all-reduced, and every rank re-filters its segment by the limit read
off the sum before the graph (distributed.sharded_assemble(auto_limit=True)); the same stderr line
and --spectrum-out / --spectrum-bins apply.
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)


def limit_arg(v):
    """--limit: an integer, or "auto" (None)"""
    if v == "auto":
        return None
    try:
        return int(v)
    except ValueError:
        raise argparse.ArgumentTypeError("%r is neither an integer nor 'auto'" % v)


def auto_limit_line(si, nbins, solid0, solid1, contigs=None):
    """the auto-limit report of rank 0 (stderr); contigs = (before, after) where both are known"""
    if si["found"]:
        line = ("auto-limit: limit %d  (spectrum lo %d  descent end %d  peak %d  floor %d)  solid k-mers %d -> %d"
                % (si["limit"], si["lo"], si["descent_end"], si["peak"], si["floor"], solid0, solid1))
        return line + ("  contigs %d -> %d" % contigs if contigs else "")
    return ("auto-limit: no limit found  (spectrum lo %d  descent end %d  peak %d of %d bins)  solid k-mers %d kept"
            % (si["lo"], si["descent_end"], si["peak"], nbins, solid0))


def main(argv=None):
    ap = argparse.ArgumentParser(description="MI355X de Bruijn unitig assembler")
    ap.add_argument("-i", "--input", required=True, help="FASTA / FASTQ read file")
    ap.add_argument("-k", type=int, default=31, help="k-mer (node) length, 1..63")
    ap.add_argument("--limit", type=limit_arg, default=1,
                    help="keep k-mers seen more than this many times; 'auto': count at limit 1 and choose the "
                         "limit from the k-mer count spectrum (every path, --sharded and several ranks included)")
    ap.add_argument("-o", "--output", default="", help="contig FASTA ('>contig%%d' records)")
    ap.add_argument("--gfa", default="", help="GFA 1 output")
    ap.add_argument("--fasta-mode", choices=["records", "lines"], default="records",
                    help="records: SeqIO-style multi-line records; lines: one read per line (src/eulercuda.py)")
    ap.add_argument("--threads", type=int, default=0, help="ingest threads (0: up to 16)")
    ap.add_argument("--backend", choices=["nccl", "gloo"], default="nccl",
                    help="torch.distributed backend (nccl = RCCL over xGMI; gloo stages through host memory)")
    ap.add_argument("--device", type=int, default=-1, help="GPU of every rank (default: LOCAL_RANK)")
    ap.add_argument("--sharded", action="store_true", help="the sharded path even with one process")
    ap.add_argument("--clip-tips", action="store_true",
                    help="clip tips (short dead-end contigs beside a longer branch) after the assembly; "
                         "one process, fused path only")
    ap.add_argument("--tip-len", type=int, default=0, help="longest tip clipped, in characters (default 2 k)")
    ap.add_argument("--tip-rounds", type=int, default=4, help="clipping rounds at most (default 4)")
    ap.add_argument("--pop-bubbles", action="store_true",
                    help="pop bubbles (of parallel short branches the best covered one stays) after the "
                         "assembly and after --clip-tips; one process, fused path only")
    ap.add_argument("--bubble-len", type=int, default=0,
                    help="longest branch popped, in characters (default 2 k; at most 65535)")
    ap.add_argument("--bubble-rounds", type=int, default=4, help="popping rounds at most (default 4)")
    ap.add_argument("--auto-limit", action="store_true",
                    help="choose the solid limit from the k-mer count spectrum of the assembly and re-filter by "
                         "it, before --clip-tips / --pop-bubbles; one process, fused path only "
                         "(--limit auto is the form that works on every path)")
    ap.add_argument("--spectrum-bins", type=int, default=1024,
                    help="bins of the count spectrum, 2 .. 4096 (default 1024; the last bin saturates)")
    ap.add_argument("--spectrum-out", default="",
                    help="with --auto-limit: write the spectrum's non-zero bins as count<TAB>k-mers lines")
    a = ap.parse_args(argv)
    limit_auto = a.limit is None
    if limit_auto:
        a.limit = 1
    if a.auto_limit and (a.sharded or int(os.environ.get("WORLD_SIZE", "1")) > 1):
        # (the spectrum of the sharded path would have to be all-reduced before the solid filter)
        print("euler_run: --auto-limit works on the one-process fused path only, not with --sharded or "
              "several ranks", file=sys.stderr)
        return 2
    if (a.auto_limit or limit_auto) and not 2 <= a.spectrum_bins <= 4096:
        print("euler_run: --spectrum-bins must be in 2 .. 4096", file=sys.stderr)
        return 2
    if a.spectrum_out and not (a.auto_limit or limit_auto):
        print("euler_run: --spectrum-out needs --auto-limit or --limit auto", file=sys.stderr)
        return 2
    if a.clip_tips and (a.sharded or int(os.environ.get("WORLD_SIZE", "1")) > 1):
        # (the junction-partitioned graph of the sharded path holds no complete link table)
        print("euler_run: --clip-tips works on the one-process fused path only, not with --sharded or "
              "several ranks", file=sys.stderr)
        return 2
    if a.clip_tips and (a.tip_len < 0 or a.tip_rounds < 1):
        print("euler_run: --tip-len must be >= 0 and --tip-rounds >= 1", file=sys.stderr)
        return 2
    if a.pop_bubbles and (a.sharded or int(os.environ.get("WORLD_SIZE", "1")) > 1):
        print("euler_run: --pop-bubbles works on the one-process fused path only, not with --sharded or "
              "several ranks", file=sys.stderr)
        return 2
    if a.pop_bubbles and (not 0 <= a.bubble_len <= 65535 or a.bubble_rounds < 1):
        print("euler_run: --bubble-len must be in 0 .. 65535 and --bubble-rounds >= 1", file=sys.stderr)
        return 2

    import torch

    import distributed
    import eulerhip
    import ingest

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0")) if a.device < 0 else a.device
    torch.cuda.set_device(local)
    t0 = time.time()
    rs = ingest.ReadSet(a.input, None, a.threads, a.fasta_mode)
    nreads = len(rs)
    lo, hi = distributed.shard_range(nreads, rank, world)
    buf, off = rs.packed(lo, hi - lo)
    rs.close()
    t_ingest = time.time() - t0
    d_buf = torch.from_numpy(buf if len(buf) else np.zeros(1, np.uint8)).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    t1 = time.time()
    sharded = world > 1 or a.sharded
    if limit_auto and not sharded:
        a.auto_limit = True
    if not sharded:
        sess = eulerhip.Session(local, stream=torch.cuda.current_stream().cuda_stream)
        sess.run_device(d_buf.data_ptr(), d_off.data_ptr(), hi - lo, a.k, a.limit, 0)
        res = None
        if a.auto_limit:
            st0 = sess.stats()
            hist = sess.kmer_spectrum(a.spectrum_bins)
            si = eulerhip.spectrum_threshold(hist)
            if a.spectrum_out and rank == 0:
                with open(a.spectrum_out, "w") as f:
                    f.write("".join("%d\t%d\n" % (c, int(hist[c])) for c in np.flatnonzero(hist)))
            if si["found"]:
                res, _ = sess.refilter(a.k, si["limit"])
                if rank == 0:
                    print(auto_limit_line(si, a.spectrum_bins, st0.n_solid, res.stats.n_solid,
                                          (st0.n_contigs, res.stats.n_contigs)), file=sys.stderr)
            elif rank == 0:
                print(auto_limit_line(si, a.spectrum_bins, st0.n_solid, st0.n_solid), file=sys.stderr)
        if a.clip_tips:
            n0 = sess.stats().n_contigs
            res, ci = sess.clip_tips(a.k, a.tip_len, a.tip_rounds)
            if rank == 0:
                print("clip-tips: rounds %d  converged %d  tip contigs %d  tip k-mers %d  contigs %d -> %d"
                      % (ci["rounds"], ci["converged"], ci["n_tip_contigs"], ci["n_tip_kmers"], n0,
                         res.stats.n_contigs), file=sys.stderr)
        if a.pop_bubbles:
            n0 = sess.stats().n_contigs
            res, pi = sess.pop_bubbles(a.k, a.bubble_len, a.bubble_rounds)
            if rank == 0:
                print("pop-bubbles: rounds %d  converged %d  bubble contigs %d  bubble k-mers %d  contigs %d -> %d"
                      % (pi["rounds"], pi["converged"], pi["n_bubble_contigs"], pi["n_bubble_kmers"], n0,
                         res.stats.n_contigs), file=sys.stderr)
        if res is None:
            res = sess.fetch(a.k)
        P = res.stats.n_positions
    else:
        import torch.distributed as dist

        if a.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group("gloo")
        eng = distributed.HipEngine(local, stream=torch.cuda.current_stream().cuda_stream)
        ai = {}
        res, P = distributed.sharded_assemble(eng, distributed.TorchComm(), d_buf, d_off, hi - lo, lo, a.k, a.limit,
                                              auto_limit=limit_auto, auto_info=ai, spectrum_bins=a.spectrum_bins)
        if limit_auto and rank == 0:
            if a.spectrum_out:
                with open(a.spectrum_out, "w") as f:
                    f.write("".join("%d\t%d\n" % cv for cv in sorted(ai["spectrum"].items())))
            print(auto_limit_line(ai, a.spectrum_bins, ai["n_solid_before"], ai["n_solid_after"]), file=sys.stderr)
    torch.cuda.synchronize()
    t_asm = time.time() - t1
    if rank == 0:
        if a.output:
            ingest.write_contigs_fasta(a.output, res, "contig%d", blank_line=False)
        if a.gfa:
            ingest.write_gfa(a.gfa, res, a.k)
        print("reads %d  k-mer positions %d  contigs %d  ingest %.2f s  assemble %.3f s  (%d GPU%s)"
              % (nreads, P, len(res.contig_offsets) - 1, t_ingest, t_asm, world, "s" if world > 1 else ""),
              file=sys.stderr)
        if not a.output and not a.gfa:
            sys.stdout.write("".join(">contig%d\n%s\n" % (i, c) for i, c in enumerate(res.contigs)))
    if sharded:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
