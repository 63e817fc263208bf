"""Dev tool: build kernel-variant library sets for same-box A/B timing.

Each variant is a scratch copy of the tree's sources (in a temporary
directory, never the product tree) with a few substitutions in
dietgpu_fork_amd/csrc, built with the Makefile into the library set
tools/ablibs/<name>/ (git-ignored).  On the GPU machine `tools/ab.py run
default tools/ablibs/<name> ...` times a set against the in-tree build and
`tools/ab.py with tools/ablibs/<name> -- <command>` runs one command under it.

The variants are experiments whose measurements DESIGN.md section 7 records
and that still apply to today's sources; those whose anchors went with later
rewrites were removed (git history has them).  A substitution that no longer
matches fails loudly, and --check lists every variant with whether it applies.
    usage: python tools/variants.py name...  |  python tools/variants.py --check"""
import os, shutil, subprocess, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ab  # noqa: E402  (tools/ab.py: the library-set copy)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = "pcompress.h"
NTST = [("encode.h", "    if (store) st8(raw + i0, make_uint2(r0, r1));", "    if (store) __builtin_nontemporal_store(u32x2{r0, r1}, (gp<u32x2>)(raw + i0));")]
# per-wave phase stamps of the three-item pipeline (round 3): stamp[(wg, iteration, wave, phase)]
STAMP3 = [
    (P, "namespace pc {", "__device__ unsigned long long g_stamp[4096 * 8 * 4 * 16];\n#define STAMP(ph) do { if (lane == 0 && itc < 8) { unsigned long long t_ = __builtin_amdgcn_s_memrealtime(); asm volatile(\"\" : \"+v\"(t_)); ((volatile unsigned long long*)g_stamp)[((blockIdx.x * 8 + itc) * 4 + w) * 16 + (ph)] = t_; } } while (0)\nnamespace pc {"),
    (P, "  uint32_t round = 0;\n", "  uint32_t round = 0;\n  uint32_t itc = 0;\n"),
    (P, "    // Segment-phase wave priority rotates", "    STAMP(0);\n    // Segment-phase wave priority rotates"),
    # the iteration head is over: the round's first input loads issue next
    (P, "#pragma unroll\n        for (uint32_t g = 0; g < uint32_t(D); ++g) load(dummy, srcL, uwL, g);", "        STAMP(11);\n#pragma unroll\n        for (uint32_t g = 0; g < uint32_t(D); ++g) load(dummy, srcL, uwL, g);"),
    (P, "    __builtin_amdgcn_s_setprio(3);\n", "    STAMP(1);\n    __builtin_amdgcn_s_setprio(3);\n"),
    (P, "    // E's word counts and L's histogram counts are in\n    __syncthreads();\n", "    // E's word counts and L's histogram counts are in\n    __syncthreads();\n    STAMP(2);\n"),
    (P, "    if (hasL) publishHist(Lw, ka);", "    if (hasL) publishHist(Lw, ka);\n    STAMP(8);"),
    (P, "    if (hasE && w == 0) lookBackE(Ew, ka);", "    STAMP(3);\n    if (hasE && w == 0) lookBackE(Ew, ka);\n    STAMP(4);"),
    (P, "      const uint32_t ep = ka.epoch;", "      STAMP(5);\n      const uint32_t ep = ka.epoch;"),
    (P, "    if (hasE && w != 0) place(Ew);", "    if (hasE && w != 0) place(Ew);\n    STAMP(6);"),
    # the decoding wave: the next item's record written
    (P, "      decodeItem(kw, ka, e, X, sN);\n", "      decodeItem(kw, ka, e, X, sN);\n      STAMP(12);\n"),
    (P, "        if (L.x == 0) {\n          asm volatile", "        STAMP(7);\n        if (L.x == 0) {\n          asm volatile"),
    (P, "      lp<u32x4> red4 = (lp<u32x4>)&hist[0];", "      STAMP(10);\n      lp<u32x4> red4 = (lp<u32x4>)&hist[0];"),
    (P, "    ++round;\n", "    STAMP(9);\n    ++itc;\n    ++round;\n"),
    ("codec.hip", "uint32_t deviceErrorCount(bool reset) {", "extern \"C\" void* dietgpu_debug_stamps() { void* p = nullptr; (void)hipGetSymbolAddress(&p, HIP_SYMBOL(g_stamp)); return p; }\n\nuint32_t deviceErrorCount(bool reset) {"),
]
# round-3 attribution variants of the three-item pipeline (outputs invalid)
V3NOENC = [(P, "const bool encOn = hasE && uwE0 != 0;", "const bool encOn = false;")]
V3NOHIST = [(P, "__hip_atomic_fetch_add(hcol + __umul24(sym, pc::kHistStride), 1u, __ATOMIC_RELAXED,\n                               __HIP_MEMORY_SCOPE_WORKGROUP);",
             "if (sym == 0x1234u) __hip_atomic_fetch_add(hcol + __umul24(sym, pc::kHistStride), 1u, __ATOMIC_RELAXED,\n                               __HIP_MEMORY_SCOPE_WORKGROUP);"),
            (P, "__hip_atomic_fetch_add(hcol + __umul24(sym, pc::kHistStride), add, __ATOMIC_RELAXED,",
             "if (sym == 0x1234u) __hip_atomic_fetch_add(hcol + __umul24(sym, pc::kHistStride), add, __ATOMIC_RELAXED,")]
V3NOSPLITST = [(P, "splitVec<FT>(v, i0, it.n, raw, myT + off, myT + off, store);", "splitVec<FT>(v, i0, it.n, raw, myT + off, myT + off, false);")]
# round-3 decode LDS attribution (outputs invalid; bench --no-verify only)
DH = "decode.h"
D_TBL = [(DH, "  for (int c = 0; c < NC; ++c) e[c] = lut[c][p[c]->x & mask];",
          "  for (int c = 0; c < NC; ++c) e[c] = lut[c][(p[c]->x & 0u) + (threadIdx.x & 63u)];")]
D_RING = [(DH, "    v[c] = q.ringLane[idx & (dec::kRing - 1)];", "    v[c] = q.ringLane[(idx & 0u) + (threadIdx.x & 31u)];")]
ENC512 = [("encode.h", "  constexpr uint32_t R = kFused ? enc::kRingFused : enc::kRing;",
           "  constexpr uint32_t R = kFused ? (FT == 0 ? enc::kRingFused : 512u) : enc::kRing;")]
SP = "sparse.hip"
NOZERO = [("upload.hip", """__global__ __launch_bounds__(256) void k_zero(uint8_t* __restrict__ dst, size_t bytes) {
  const size_t stride = size_t(gridDim.x) * 256;
  const size_t i0 = size_t(blockIdx.x) * 256 + threadIdx.x;
  if ((reinterpret_cast<uintptr_t>(dst) | bytes) % 16 == 0) {
    uint4* d = reinterpret_cast<uint4*>(dst);
    for (size_t i = i0; i < bytes / 16; i += stride) d[i] = make_uint4(0, 0, 0, 0);
  } else {
    for (size_t i = i0; i < bytes; i += stride) dst[i] = 0;
  }
}
""", ""), ("upload.hip", """  const size_t units = (reinterpret_cast<uintptr_t>(dst) | bytes) % 16 == 0 ? bytes / 16 : bytes;
  const uint32_t grid = uint32_t(std::min<size_t>(1024, (units + 255) / 256));
  k_zero<<<grid, 256, 0, s>>>(static_cast<uint8_t*>(dst), bytes);
  HIP_LAUNCH_CHECK();""", """  HIP_CHECK(hipMemsetAsync(dst, 0, bytes, s));""")]
# test-only: k_pcompress workgroups start in about
# reverse index order within every 64 (skewDelay, 1 us steps), so its
# look-back and element-log waits meet late-starting lower workgroups; run
# by tools/skew_check.sh against tests/test_gpu_progress.py.  The product
# kernel carries no hook (a one-line hook tipped its register allocation,
# DESIGN.md section 7).
PSKEW = [(P, "  __syncthreads();  // histogram zeroed, records written\n",
          "  if (tid == 0) skewDelay(100);\n  __syncthreads();  // histogram zeroed, records written\n")]
VARS = {
    "pskew": PSKEW,
    # decoder output store cache policies (global_store_dwordx4 with the
    # policy bits in the instruction; "plain" = none)
    **{f"sp_{name}": [("device.h", """__device__ __forceinline__ void st16nt(gp<void> p, uint4 v) {
  __builtin_nontemporal_store(u32x4{v.x, v.y, v.z, v.w}, (gp<u32x4>)p);
}""", """__device__ __forceinline__ void st16nt(gp<void> p, uint4 v) {
  asm volatile("global_store_dwordx4 %%0, %%1, off %s" :: "v"(p), "v"(u32x4{v.x, v.y, v.z, v.w}) : "memory");
}""" % pol)] for name, pol in (("plain", ""), ("sc0", "sc0"), ("sc1", "sc1"), ("sc01", "sc0 sc1"),
                                ("ntsc1", "nt sc1"), ("ntsc0", "nt sc0"), ("nt", "nt"))},
    # round 5: one segment of loads in flight (a shallower memory queue for
    # the hand-off window's loads, which queue behind the CU's streaming)
    "pcd1": [(P, "  constexpr int D = 2;", "  constexpr int D = 1;")],
    # round 5: the quotient's shift operand read from byte 3 of the table
    # entry by SDWA (one VALU per encode step fewer)
    "sdwa": [("encode.h", "  const uint32_t q = __umulhi(x, e.y) >> (e.w >> 24);",
              """  uint32_t q;
  asm("v_lshrrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD"
      : "=v"(q) : "v"(e.w), "v"(__umulhi(x, e.y)));""")],
    "pc128": [("compress_plan.h", "constexpr uint32_t kMaxTeam = 32;", "constexpr uint32_t kMaxTeam = 128;")],
    # sparse count diagnostics (timing only: archives wrong)
    "sp_nolds": [(SP, "      if (i + 1 == n && gap) count(W(0));\n      if (v != W(0)) count(v);", "      if (v == W(0x12345u)) count(v);")],
    "sp_nostage": [(SP, "    if (i + 1 == n && gap) {\n      st[dst] = W(0);\n      if (v != W(0)) st[dst + 1] = v;\n    } else if (v != W(0)) {\n      st[dst] = v;\n    }", "    if (v == W(0x12345u)) st[dst] = v;")],
    "slp0": [(P, "        if (spins) __builtin_amdgcn_s_sleep(2);", "")],
    "slp1": [(P, "        if (spins) __builtin_amdgcn_s_sleep(2);", "        if (spins) __builtin_amdgcn_s_sleep(1);")],
    "pcd3": [(P, "  constexpr int D = 2;", "  constexpr int D = 3;")],
    "nozero": NOZERO,
    "hcl": [(P, "lp<uint32_t> hcol = (lp<uint32_t>)&hist[l % pc::kHistCols];", "lp<uint32_t> hcol = (lp<uint32_t>)&hist[laneNow() % pc::kHistCols];")],
    "hcx": [(P, "lp<uint32_t> hcol = (lp<uint32_t>)&hist[l % pc::kHistCols];", "lp<uint32_t> hcol = (lp<uint32_t>)&hist[(l + (halfNow() ? 6u : 0u)) % pc::kHistCols];")],
    "kf8": [(P, "constexpr uint32_t kFirst = 4;                         // loaded before the barrier", "constexpr uint32_t kFirst = 8;                         // loaded before the barrier")],
    "encprio": [("encode.h", "    // every wave's slot stores are complete before other waves copy them\n    asm volatile(\"s_waitcnt vmcnt(0)\" ::: \"memory\");", "    __builtin_amdgcn_s_setprio(2);\n    // every wave's slot stores are complete before other waves copy them\n    asm volatile(\"s_waitcnt vmcnt(0)\" ::: \"memory\");")],
    "d3": [(P, "  constexpr int D = 2;", "  constexpr int D = 3;")],
    "ntst": NTST,
    "stamp3": STAMP3,
    "v3noenc": V3NOENC,
    "v3nohist": V3NOHIST,
    "v3nosplitst": V3NOSPLITST,
    "v3noencnohist": V3NOENC + V3NOHIST,
    "enc512": ENC512,
    "d_tbl": D_TBL,
    "d_ring": D_RING,
    "base": [],
    "hist2x": [(P, "__hip_atomic_fetch_add(hcol + __umul24(sym, pc::kHistStride), 1u, __ATOMIC_RELAXED,\n                               __HIP_MEMORY_SCOPE_WORKGROUP);",
                "__hip_atomic_fetch_add(hcol + __umul24(sym, pc::kHistStride), 1u, __ATOMIC_RELAXED,\n                               __HIP_MEMORY_SCOPE_WORKGROUP);\n        __hip_atomic_fetch_add(hcol + __umul24(sym, pc::kHistStride), 1u, __ATOMIC_RELAXED,\n                               __HIP_MEMORY_SCOPE_WORKGROUP);")],
    "nosplitst": [(P, "splitVec<FT>(v, i0, it.n, raw, myT + off, myT + off, store);", "splitVec<FT>(v, i0, it.n, raw, myT + off, myT + off, false);")],
}
EH = "encode.h"
# cost probes (wrong archives): the encode step without its ring write /
# without the step at all (table reads kept)
VARS["noemit"] = [(EH, 'asm volatile("s_and_saveexec_b64 %0, %1\\n\\tds_write_b16', 'if (0) asm volatile("s_and_saveexec_b64 %0, %1\\n\\tds_write_b16')]
# ring stores without the exec mask: non-writers store to a per-thread
# discard slot (v_cndmask on the vote), so a step's store no longer orders
# the next step's VALU behind an exec restore
TRASH = [
    (EH, "  gp<uint16_t> out[2];     // per half: slot data\n};",
     "  gp<uint16_t> out[2];     // per half: slot data\n  uint32_t trash;          // LDS byte address of this thread's discard slot\n};"),
    (EH, """  uint64_t sav;
  asm volatile("s_and_saveexec_b64 %0, %1\\n\\tds_write_b16 %2, %3\\n\\ts_mov_b64 exec, %0"
               : "=&s"(sav)
               : "s"(vote), "v"(ringAddr), "v"(p.x)
               : "memory", "scc");""",
     """  uint32_t wa;
  asm volatile("v_cndmask_b32_e64 %0, %1, %2, %3\\n\\tds_write_b16 %0, %4"
               : "=&v"(wa)
               : "v"(p.trash), "v"(ringAddr), "s"(vote), "v"(p.x)
               : "memory");"""),
    (EH, "  __shared__ uint32_t cwE[Cfg::kBlocksPerWG];",
     "  __shared__ __attribute__((aligned(16))) uint16_t trashS[enc::kThreads];\n  __shared__ uint32_t cwE[Cfg::kBlocksPerWG];"),
    (EH, "    p.ringLane = p.ring + (hv & R);\n",
     "    p.ringLane = p.ring + (hv & R);\n    p.trash = uint32_t(size_t((lp<uint16_t>)&trashS[threadIdx.x]));\n"),
    (P, "  __shared__ __attribute__((aligned(16))) uint16_t rings[pc::kBlocksPerItem * pc::kRing];",
     "  __shared__ __attribute__((aligned(16))) uint16_t rings[pc::kBlocksPerItem * pc::kRing];\n  __shared__ __attribute__((aligned(16))) uint16_t trashS[pc::kThreads];"),
    (P, "    p.ringLane = p.ring + (hv & pc::kRing);\n",
     "    p.ringLane = p.ring + (hv & pc::kRing);\n    p.trash = uint32_t(size_t((lp<uint16_t>)&trashS[threadIdx.x]));\n"),
]
VARS["trash"] = TRASH
# fp64 k_coalesce granularity (blocks per workgroup; 4 is the product's)
VARS["bpw8"] = [("codec.hip", "      const uint32_t bpw = 4;", "      const uint32_t bpw = 8;")]
VARS["bpw16"] = [("codec.hip", "      const uint32_t bpw = 4;", "      const uint32_t bpw = 16;")]
VARS["noexec"] = [(EH, 'asm volatile("s_and_saveexec_b64 %0, %1\\n\\tds_write_b16 %2, %3\\n\\ts_mov_b64 exec, %0"',
                   'asm volatile("s_mov_b64 %0, %1\\n\\tds_write_b16 %2, %3"')]
VARS["noidx"] = [(EH, "const uint32_t ringAddr = uint32_t(size_t(p.ringLane + (idx & (kRing - 1))));",
                  "(void)idx; const uint32_t ringAddr = uint32_t(size_t(p.ringLane + (__builtin_amdgcn_mbcnt_lo(~0u, 0u) & 31)));")]
VARS["nostep"] = [(EH, "for (int s = 0; s < S; ++s) encStep<kMask, R>(st[s], vd[u], E[u][s], hv);",
                   "for (int s = 0; s < S; ++s) st[s].x += E[u][s].z;"),
                  (P, "        encStep<kMask, pc::kRing>(p, !kMask || (t0 + u) * 32 + l < uw, Ev[u], hv);",
                   "        p.x += Ev[u].z;")]
# round 6: the decoder's archive reads streamed (read once per call): raw
# float bytes / compressed words as nontemporal loads
DEC = "decode.h"
DNT_RAW = [(DEC, "      const uint2 a = ld8(raw + i0);",
            "      const u32x2 a_ = __builtin_nontemporal_load((gp<const u32x2>)(raw + i0)); const uint2 a = make_uint2(a_.x, a_.y);"),
           (DEC, "      const uint4 a = ld16(raw + 2 * i0);", "      const uint4 a = ld16nt(raw + 2 * i0);")]
DNT_RING = [(DEC, "  if (vec) return *(gp<const u32x2>)p;", "  if (vec) return __builtin_nontemporal_load((gp<const u32x2>)p);")]
VARS["dnt_raw"] = DNT_RAW
VARS["dnt_ring"] = DNT_RING
VARS["dnt_both"] = DNT_RAW + DNT_RING


def applies(subs):
    return all(os.path.exists(f"{REPO}/dietgpu_fork_amd/csrc/{f}") and
               open(f"{REPO}/dietgpu_fork_amd/csrc/{f}").read().count(a) >= 1 for f, a, _ in subs)


def build(name):
    root = tempfile.mkdtemp(prefix=f"var_{name}_")
    try:
        shutil.copytree(f"{REPO}/dietgpu_fork_amd/csrc", f"{root}/dietgpu_fork_amd/csrc")
        for d in ("include", "tests"):  # the Makefile reads ../../include and ../../tests/cpp
            os.symlink(f"{REPO}/{d}", f"{root}/{d}")
        for f, a, b in VARS[name]:
            p = f"{root}/dietgpu_fork_amd/csrc/{f}"
            s = open(p).read()
            assert s.count(a) >= 1, (name, a[:60])
            open(p, "w").write(s.replace(a, b))
        jobs = min(16, os.cpu_count() or 8)
        subprocess.check_call(["make", "-s", f"-j{jobs}", "-C", f"{root}/dietgpu_fork_amd/csrc"])
        os.makedirs(f"{REPO}/tools/ablibs/{name}", exist_ok=True)
        ab.swap_in(f"{root}/dietgpu_fork_amd/_lib", f"{REPO}/tools/ablibs/{name}")
    finally:
        shutil.rmtree(root, ignore_errors=True)
    print("built", name)


if __name__ == "__main__":
    if sys.argv[1:] == ["--check"]:
        for name, subs in VARS.items():
            print(f"{name:32s} {'applies' if applies(subs) else 'stale (anchors gone)'}")
    else:
        for name in sys.argv[1:]:
            build(name)
