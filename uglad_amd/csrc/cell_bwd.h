// Body of the cell backward kernel, included twice by glad_kernels.hip (inside namespace uglad, between cell_fwd.h and theta0.h; every
// unit holds both templates, the per-NT units instantiate the first and the -DUGLAD_TU_GS units the second):
//   UGLAD_CELL_BWD_GS 0: cell_bwd_kernel     -- the 42 parameter gradients and dL/dZ_k;
//   UGLAD_CELL_BWD_GS 1: cell_bwd_gs_kernel  -- the same, and also dL/dS of every step accumulated into gS (M, D, D), which the caller zeroed
//                        before the pass: gS += G_B / lam_k (b_k = S / lam_k - Z_k) + the rhoNN input gradient of the S feature.  The thread that
//                        owns the upper-triangle entry (i, j) adds both terms to gS_ij and mirrors the sum into gS_ji, so gS stays exactly
//                        symmetric; everything else is computed by the same code.
// One body for both, switched by the preprocessor rather than a bool template parameter on a __device__ body: called from two kernels,
// the device function is simplified on its own before it is inlined, and cell_bwd_kernel came out with other register and spill figures
// (scripts/kernel_meta.py, NT = 2: 177 instead of 181 VGPRs, 51 instead of 9 SGPR spills).  Included textually, cell_bwd_kernel is token
// for token the kernel it was; the gS instantiations live in translation units of their own (UGLAD_TU_GS), since next to cell_bwd_kernel<3>
// they moved its SGPR spills from 78 to 80.
template <int NT>
__global__ __launch_bounds__(kThreads) void UGLAD_CELL_BWD_NAME(
    const float* __restrict__ Gnext, const float* __restrict__ S, const float* __restrict__ Zin,
    const float* __restrict__ half, const float* __restrict__ U, const float* __restrict__ beta,
    const float* __restrict__ lam_ptr, const float* __restrict__ params, float* __restrict__ Gout,
    float* __restrict__ grad_rho_partial, float* __restrict__ glam_partial, float* __restrict__ gws, int D, int mode,
#if UGLAD_CELL_BWD_GS
    int gs, int k_count, int lam_stride, float* __restrict__ gS) {
#else
    int gs, int k_count, int lam_stride) {
#endif
  constexpr int DP = NT * 32, LD = DP + 1;
  UGLAD_BIG_BUFFERS(sX, DP * LD, sY, DP * LD, gws)  // U ; G -> G_half -> T -> C o F -> T2
  __shared__ float s_beta[DP], s_r[DP];
  __shared__ __attribute__((aligned(16))) float s_a0[DP], s_aN[DP];  // NS10: a_i^(0) and a_i^(10), all that K_ij needs (ns_divided_difference)
  __shared__ float s_red[8];
  __shared__ float s_g[kWaves][kNRho + 1];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const size_t base = (size_t)blockIdx.x * D * D;
  const float* Sm = S + base;
  const float* Gm = Gnext + base;
  float* Go = Gout + base;
  const int grp = blockIdx.x / gs;
  params += (size_t)grp * kNParam;
  // k_count consecutive steps k, k-1, ... of the unrolled pass in ONE launch (DP <= 128 only): the pointers name step k, step k - s sits
  // s slabs (gridDim.x matrices) below.  dL/dZ stays in LDS from one step to the next -- the two big buffers swap roles -- the 28 rhoNN
  // gradient sums stay in registers, and only the last step writes G_out.  k_count = 1 is the per-step entry point.
  const size_t step_mdd = (size_t)gridDim.x * D * D, step_md = (size_t)gridDim.x * D;
  // The 28 rhoNN gradient sums.  kPackA: phase A runs the rhoNN backward of two entries at a time (rho_backward2) and the sums are kept as
  // pairs, g2[q].x over a thread's even entries and g2[q].y over its odd ones, added once in front of the final reduction; 28 more registers
  // across the whole step loop.  NT = 8 (224 VGPRs with the sums held once) keeps them once and the backward entry by entry.
  constexpr bool kPackA = NT <= 7;
  float g[kNRho];
  [[maybe_unused]] v2f g2[kNRho];
#pragma unroll
  for (int q = 0; q < kNRho; ++q) g[q] = 0.f, g2[q] = splat2(0.f);
  // The upper-triangle entries of a thread (entry e = tid + kThreads q, as in the forward cell) are the same in every step.  DP <= 128: they are
  // worked out once, here, into s_ent[q][tid] = (i << 8) | j, 0xffff where there is none ([q][tid]: a wave reads 64 consecutive shorts), and
  // phase A and the G_out assembly of every step read them back in the order q = 0, 1, ... they were walked in -- the summation order of the 28
  // rhoNN sums and of dL/dlam.  Beyond (66 KB of table), the walk is redone in each of the two phases.
  constexpr int kMaxQ = ((DP / 2) * (DP + 1) + kThreads - 1) / kThreads;
  constexpr bool kPre = DP <= 128;          // all entries of a thread in registers at once
  constexpr int kQ = kPre ? kMaxQ : 8;      // entries per thread and pass
  constexpr int kIShift = kPre ? 8 : 16, kJMask = (1 << kIShift) - 1;
  const int D1 = D + 1, total = ((D + 1) / 2) * D1;
  const int sp = kThreads / D1, sc = kThreads - sp * D1;
  auto entry = [&](int e, int p, int c) -> int {  // (i << kIShift) | j of entry (pair p, offset c), -1 when there is none
    if (e >= total) return -1;
    if (c < D - p) return (p << kIShift) | (p + c);
    const int i = D - 1 - p;
    return (i == p) ? -1 : ((i << kIShift) | (i + (c - (D - p))));
  };
  auto advance = [&](int& p, int& c) {
    c += sc;
    p += sp;
    if (c >= D1) {
      c -= D1;
      ++p;
    }
  };
  __shared__ unsigned short s_ent[kPre ? kMaxQ : 1][kPre ? kThreads : 1];
  if constexpr (kPre) {
    int p = tid / D1, c = tid - p * D1;
    for (int q = 0; q < kMaxQ; ++q) {
      s_ent[q][tid] = (unsigned short)entry(tid + kThreads * q, p, c);  // (read back by this thread alone: no barrier)
      advance(p, c);
    }
  }
#pragma unroll 1
  for (int s = 0; s < k_count; ++s) {
    const bool first = (s == 0), last = (s == k_count - 1);
    const int tid = opaque_v(threadIdx.x), lane = tid & 63;  // (shadow the outer ones: nothing per-thread is hoisted)
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // (scalar: the tile indices derived from it live in SGPRs)
    const float* Zm = Zin + base - s * step_mdd;
    const float* Hm = half + base - s * step_mdd;
    const float* Um = U + base - s * step_mdd;
    const float* bm = beta + (size_t)blockIdx.x * D - s * step_md;
    const float lam = lam_ptr[(long)grp - (long)s * lam_stride];
    const float c4 = 4.0f / lam, inv_lam2 = 1.0f / (lam * lam);

    KSTAMP(0);
    // U -> sX, and in the first step G_next -> sY (afterwards G is there already): row-major, coalesced.
    // The loads are unconditional (a clamped address, the value selected afterwards): with `in ? load : 0` the compiler put every load
    // behind its own branch and an s_waitcnt vmcnt(0), one round trip after the other (30 k instead of 17 k ticks for this phase).
    // (Explicit loops, not a helper taking the destination as a pointer: through a pointer parameter the LDS stores become flat stores
    // that may alias the loads, and the loop serialises completely -- 137 k ticks.)
    //  * D == DP and 16-byte-aligned matrices (wave-uniform test): the matrix is one contiguous block, fetched as 16-byte pieces with no
    //    index arithmetic.  At DP = 128 a thread issues all its 8 loads (first step: 16, U and G) and waits once; beyond, 8 per batch.
    //  * otherwise 4-byte loads, 8 per batch (first step: 16), the position (i, k) and the offset advanced from load to load instead of a
    //    division and a 64-bit multiply-add per element, the offsets 32-bit (load_at): the 8 requests of a batch are in flight together.
    constexpr int kV4 = DP * DP / 4, kC4 = DP / 4;
    constexpr bool kFull4 = kV4 % (8 * kThreads) == 0, kFull1 = (DP * DP) % (8 * kThreads) == 0;  // no partial batch: no test per element
    const bool vec16 = (D == DP) && (((reinterpret_cast<size_t>(U) | (first ? reinterpret_cast<size_t>(Gnext) : 0)) & 15) == 0);
    if (vec16) {
      if (first) {
        for (int v0 = 0; v0 < kV4; v0 += 8 * kThreads) {
          f4 u[8], gv[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const int idx = v0 + q * kThreads + tid;
            const unsigned at = (kFull4 || idx < kV4) ? 16u * idx : 0u;
            u[q] = load_at<f4>(Um, at);
            gv[q] = load_at<f4>(Gm, at);
          }
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const int idx = v0 + q * kThreads + tid;
            if (kFull4 || idx < kV4) {
              const int i = idx / kC4, k = 4 * (idx - i * kC4);
              sX[i * LD + k] = u[q].x, sX[i * LD + k + 1] = u[q].y, sX[i * LD + k + 2] = u[q].z, sX[i * LD + k + 3] = u[q].w;
              sY[i * LD + k] = gv[q].x, sY[i * LD + k + 1] = gv[q].y, sY[i * LD + k + 2] = gv[q].z, sY[i * LD + k + 3] = gv[q].w;
            }
          }
        }
      } else {
        for (int v0 = 0; v0 < kV4; v0 += 8 * kThreads) {
          f4 u[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const int idx = v0 + q * kThreads + tid;
            u[q] = load_at<f4>(Um, (kFull4 || idx < kV4) ? 16u * idx : 0u);
          }
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const int idx = v0 + q * kThreads + tid;
            if (kFull4 || idx < kV4) {
              const int i = idx / kC4, k = 4 * (idx - i * kC4);
              sX[i * LD + k] = u[q].x, sX[i * LD + k + 1] = u[q].y, sX[i * LD + k + 2] = u[q].z, sX[i * LD + k + 3] = u[q].w;
            }
          }
        }
      }
    } else {
      // element idx = tid + kThreads * (number of the load) of the padded DP x DP matrix sits at (i, k); one load further it is
      // (i + si, k + sk), carried into the next row where k passes DP
      constexpr int si = kThreads / DP, sk = kThreads - si * DP;
      int i = tid / DP, k = tid - i * DP;
      int off = i * D + k;  // of (i, k) in the D x D matrix
      const int soff = si * D + sk, wrap = D - DP;
      if (first) {
        for (int idx0 = 0; idx0 < DP * DP; idx0 += 8 * kThreads) {
          float u[8], gv[8];
          int dst[8];
          bool in[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            in[q] = (kFull1 || idx0 + q * kThreads + tid < DP * DP) && i < D && k < D;
            const unsigned at = in[q] ? 4u * off : 0u;
            u[q] = load_at<float>(Um, at);
            gv[q] = load_at<float>(Gm, at);
            dst[q] = i * LD + k;
            i += si, k += sk, off += soff;
            if (k >= DP) k -= DP, ++i, off += wrap;
          }
          __builtin_amdgcn_sched_barrier(0);  // (else the scheduler pairs every load with its store and waits for each in turn)
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            if (kFull1 || idx0 + q * kThreads + tid < DP * DP) {
              sX[dst[q]] = in[q] ? u[q] : 0.f;
              sY[dst[q]] = in[q] ? gv[q] : 0.f;
            }
          }
        }
      } else {
        for (int idx0 = 0; idx0 < DP * DP; idx0 += 8 * kThreads) {
          float u[8];
          int dst[8];
          bool in[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            in[q] = (kFull1 || idx0 + q * kThreads + tid < DP * DP) && i < D && k < D;
            u[q] = load_at<float>(Um, in[q] ? 4u * off : 0u);
            dst[q] = i * LD + k;
            i += si, k += sk, off += soff;
            if (k >= DP) k -= DP, ++i, off += wrap;
          }
          __builtin_amdgcn_sched_barrier(0);  // (else the scheduler pairs every load with its store and waits for each in turn)
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            if (kFull1 || idx0 + q * kThreads + tid < DP * DP) sX[dst[q]] = in[q] ? u[q] : 0.f;
          }
        }
      }
    }
    // DP <= 128: phase A's operands from global memory (H, Z, S of every entry of this thread) are requested here, in front of the spectrum
    // set-up, whose two block sums cost four barriers, and waited for behind it.  Clamped addresses.  The set-up's own operand, beta of this
    // thread, is requested first: loads return in order, and behind the 51 its wait would be a wait for all of them.
    const float be_ld = load_at<float>(bm, (tid < D) ? 4u * (unsigned)tid : 0u);
    [[maybe_unused]] float hx_a[kQ], zz_a[kQ], sv_a[kQ];
    if constexpr (kPre) {
      int ea[kQ];
#pragma unroll
      for (int u = 0; u < kQ; ++u) ea[u] = (int)(short)s_ent[u][tid];
#pragma unroll
      for (int u = 0; u < kQ; ++u) {
        // (opaque: left visible, the select becomes a branch around the address, behind a wait for this entry's table read alone)
        const unsigned at = (unsigned)opaque_v((ea[u] >= 0) ? 4 * ((ea[u] >> kIShift) * D + (ea[u] & kJMask)) : 0);
        hx_a[u] = load_at<float>(Hm, at);
        zz_a[u] = load_at<float>(Zm, at);
        sv_a[u] = load_at<float>(Sm, at);
      }
    }
    float a2 = 0.f;
    if (tid < D) {
      const float be = be_ld;
      const float al = fmaf(be, be, c4);
      a2 = al * al;
    }
    const float nrmA = sqrtf(block_sum(a2, s_red));
    float r2 = 0.f;
    if (tid < DP) {
      float be = 0.f, r = 1.f;
      if (tid < D) {
        be = be_ld;
        r = sqrt_spectrum(be, c4, nrmA, mode);
        r2 = r * r;
      }
      s_beta[tid] = be;
      s_r[tid] = r;
    }
    const float nrmR = sqrtf(block_sum(r2, s_red));
    if (mode == UGLAD_SQRT_NS10 && tid < DP) {
      float a = s_r[tid] / nrmR;
      s_a0[tid] = a;
#pragma unroll
      for (int it = 0; it < kNsIters; ++it) a = 0.5f * a * (3.f - a * a);
      s_aN[tid] = a;
    }
    __syncthreads();

    KSTAMP(1);
    // ---- phase A: rhoNN + threshold backward on the upper triangle (entry e = tid + kThreads q, as in the forward cell)
    using TU = Tiles<NT, true>;
    [[maybe_unused]] const int p0 = tid / D1, c0 = tid - p0 * D1;  // where this thread's walk starts (DP > 128 only: below, the table)
    float gz[kQ];  // dL/dZ_in, direct part (through rhoNN's third input); DP > 128: parked in G_out's upper triangle instead
    {
      [[maybe_unused]] int p = p0, c = c0;
      for (int q0 = 0; q0 < kMaxQ; q0 += kQ) {
        int pk[kQ];
        float hx[kQ], zz[kQ], gn[kQ], sv[kQ];
        if constexpr (kPre) {
          // the pass's indices together, then every operand from a clamped address (H, Z, S: requested in front of the spectrum set-up), no
          // branch per entry, the two LDS reads of every G entry issued before the first of them is waited for
#pragma unroll
          for (int u = 0; u < kQ; ++u) pk[u] = (int)(short)s_ent[u][tid];
          float gt[kQ];
#pragma unroll
          for (int u = 0; u < kQ; ++u) {
            const int i = pk[u] >> kIShift, j = pk[u] & kJMask;
            const bool in = pk[u] >= 0;
            gn[u] = sY[opaque_v(in ? i * LD + j : 0)];  // (opaque: left visible, the select becomes a branch around the two reads)
            gt[u] = sY[opaque_v(in ? j * LD + i : 0)];
          }
          // an entry that does not exist keeps the finite operands of the clamped addresses (entry (0, 0)): below it has g_rho = 0 and weight 0
          static_assert(kPackA || !kPre, "the tabled entries go with the packed backward");
#pragma unroll
          for (int u = 0; u < kQ; ++u) {
            const int i = pk[u] >> kIShift, j = pk[u] & kJMask;
            hx[u] = hx_a[u], zz[u] = zz_a[u], sv[u] = sv_a[u];
            gn[u] = (i == j) ? gn[u] : 0.5f * (gn[u] + gt[u]);
          }
        } else {
#pragma unroll
          for (int u = 0; u < kQ; ++u) {
            pk[u] = (q0 + u < kMaxQ) ? entry(tid + kThreads * (q0 + u), p, c) : -1;
            advance(p, c);
            const int i = pk[u] >> kIShift, j = pk[u] & kJMask;
            const bool in = pk[u] >= 0;
            hx[u] = in ? Hm[i * D + j] : 0.f;
            zz[u] = in ? Zm[i * D + j] : 0.f;
            sv[u] = in ? Sm[i * D + j] : 0.f;
            gn[u] = in ? ((i == j) ? sY[i * LD + j] : 0.5f * (sY[i * LD + j] + sY[j * LD + i])) : 0.f;
          }
        }
        constexpr int kQ2 = (kQ + 1) / 2;
        if constexpr (kPackA) {
          [[maybe_unused]] const int tid_a = opaque_v(tid);
          // forward activations and backward of two entries at a time on the packed fp32 pipe: rho_backward2 takes the pair as rho_forward2
          // left it and adds it to the two halves of g2.  No branch per entry: one that does not exist (also the missing partner of the odd
          // one out) or is inactive has g_rho = 0 and weight 0 and finite operands, so it adds exact zeros to every sum and its gh and gz
          // are 0; one that does not exist stores its gh to the padding column, which nobody reads.
#pragma unroll
          for (int h = 0; h < kQ2; ++h) {
            const int u0 = 2 * h, u1 = (2 * h + 1 < kQ) ? 2 * h + 1 : 2 * h;
            const bool has1 = 2 * h + 1 < kQ;
            // (DP <= 128: the pair's indices from the table again, through tid_a, rather than 17 registers held from the reads above)
            const int e0 = kPre ? (int)(short)s_ent[kPre ? u0 : 0][kPre ? tid_a : 0] : pk[u0];
            const int e1 = kPre ? (int)(short)s_ent[kPre ? u1 : 0][kPre ? tid_a : 0] : pk[u1];
            const bool in0 = e0 >= 0, in1 = has1 && e1 >= 0;
            const int i0 = e0 >> kIShift, j0 = e0 & kJMask, i1 = e1 >> kIShift, j1 = e1 & kJMask;
            const v2f x = {hx[u0], has1 ? hx[u1] : 0.f}, s2 = {sv[u0], has1 ? sv[u1] : 0.f}, z2 = {zz[u0], has1 ? zz[u1] : 0.f};
            const v2f gn2 = {gn[u0], has1 ? gn[u1] : 0.f};
            RhoAct2 act2;
            rho_forward2(params, x, s2, z2, act2);
            const bool on0 = in0 && fabsf(x.x) > act2.rho.x, on1 = in1 && fabsf(x.y) > act2.rho.y;
            const v2f gact = {on0 ? gn2.x : 0.f, on1 ? gn2.y : 0.f};
            // -sign(x) g for an active entry (|x| > rho >= 0: x is not 0)
            const v2f g_rho = {on0 ? ((x.x > 0.f) ? -gn2.x : gn2.x) : 0.f, on1 ? ((x.y > 0.f) ? -gn2.y : gn2.y) : 0.f};
            const v2f wgt = {on0 ? ((i0 == j0) ? 1.f : 2.f) : 0.f, on1 ? ((i1 == j1) ? 1.f : 2.f) : 0.f};
            v2f gx1, gx3;
            rho_backward2(params, x, s2, z2, act2, g_rho, wgt, g2, gx1, gx3);
            // (opaque: the sums and dL/dZ's direct part exist here, in registers -- left to the compiler, what is only needed behind the four
            // products is computed there, and its operands, three and more registers per value, are kept or spilled until then)
#pragma unroll
            for (int q = 0; q < kNRho; ++q) g2[q] = opaque_f2(g2[q]);
            gx3 = opaque_f2(gx3);
#if UGLAD_CELL_BWD_GS
            // (upper triangle; mirrored with the G_B term at the end of the step)
            if (in0) gS[base + i0 * D + j0] += rho_backward_col(params, act2.half(0), g_rho.x, 1);
            if (in1) gS[base + i1 * D + j1] += rho_backward_col(params, act2.half(1), g_rho.y, 1);
#endif
            const v2f gh = gact + gx1;
            // (opaque, as for the reads: left visible, the select becomes a branch around the two stores)
            sY[opaque_v(in0 ? i0 * LD + j0 : DP)] = gh.x;
            sY[opaque_v(in0 ? j0 * LD + i0 : DP)] = gh.x;
            if (has1) {
              sY[opaque_v(in1 ? i1 * LD + j1 : DP)] = gh.y;
              sY[opaque_v(in1 ? j1 * LD + i1 : DP)] = gh.y;
            }
            if constexpr (kPre) {
              gz[u0] = gx3.x;
              if (has1) gz[u1] = gx3.y;
            } else {
              if (in0) Go[i0 * D + j0] = gx3.x;
              if (in1) Go[i1 * D + j1] = gx3.y;
            }
          }
        } else {
        // forward activations of two entries at a time on the packed fp32 pipe, the backward entry by entry (kPackA: the 28 more
        // accumulators of the packed form do not fit this instantiation's registers)
#pragma unroll
        for (int h = 0; h < kQ2; ++h) {
          const int u0 = 2 * h, u1 = (2 * h + 1 < kQ) ? 2 * h + 1 : 2 * h;
          const bool has1 = 2 * h + 1 < kQ;
          if (!has1 && pk[u0] < 0) continue;  // (the odd one out exists on a few threads only)
          RhoAct2 act2;
          rho_forward2(params, (v2f){hx[u0], has1 ? hx[u1] : 0.f}, (v2f){sv[u0], has1 ? sv[u1] : 0.f},
                       (v2f){zz[u0], has1 ? zz[u1] : 0.f}, act2);
#pragma unroll
          for (int c2 = 0; c2 < 2; ++c2) {
            const int u = c2 ? u1 : u0;
            if ((c2 == 0 || has1) && pk[u] >= 0) {
              const int i = pk[u] >> kIShift, j = pk[u] & kJMask;
              const RhoAct act = act2.half(c2);
              const float x = hx[u];
              const bool active = fabsf(x) > act.rho;
              const float sgn = (x > 0.f) ? 1.f : ((x < 0.f) ? -1.f : 0.f);
              const float g_rho = active ? -sgn * gn[u] : 0.f;
              float gx1, gx3;
              rho_backward(params, x, sv[u], zz[u], act, g_rho, (i == j) ? 1.f : 2.f, g, gx1, gx3);
#if UGLAD_CELL_BWD_GS
              gS[base + i * D + j] += rho_backward_col(params, act, g_rho, 1);  // (upper triangle; mirrored with the G_B term at the end of the step)
#endif
              const float gh = (active ? gn[u] : 0.f) + gx1;
              sY[i * LD + j] = gh;
              sY[j * LD + i] = gh;
              if (kPre) gz[u] = gx3;
              else Go[i * D + j] = gx3;
            }
          }
        }
        }
      }
    }
    __syncthreads();

    KSTAMP(2);
    using T = Tiles<NT, false>;
    {
      f32x16 acc[T::kPerWave];
      // T1 = G_half U
      gemm_lds<NT, false, false, false>(sY, sX, acc);
      __syncthreads();
      store_tiles<NT>(sY, acc);
    }
    __syncthreads();
    KSTAMP(3);
    float glam = 0.f;
    {
      // C = U^T T1 (symmetric: upper tiles) ; Y = C o F mirrored ; diagonal term of dL/dlam
      f32x16 acc[TU::kPerWave];
      gemm_lds<NT, true, false, true>(sX, sY, acc);
      __syncthreads();
      KSTAMP(4);
#pragma unroll
      for (int n = 0; n < TU::kPerWave; ++n) {
        const int t = w + kWaves * n;
        if (t < TU::kCount) {
          int I, J;
          TU::ij(t, I, J);
          const int j = J * 32 + (lane & 31);
          const float a0j = s_a0[j], aNj = s_aN[j];
          const float rj = s_r[j], bj = s_beta[j];
          const float inv_2nrmR = 1.0f / (2.f * nrmR);
#pragma unroll
          for (int e4 = 0; e4 < 4; ++e4) {  // accumulator entries 4 e4 .. 4 e4 + 3 sit in four consecutive rows
            const int i0 = I * 32 + 8 * e4 + 4 * (lane >> 5);
            float Kr[4];
            if (mode == UGLAD_SQRT_EXACT) {
#pragma unroll
              for (int r = 0; r < 4; ++r) Kr[r] = 1.0f / (s_r[i0 + r] + rj);
            } else {
              const f4 a0 = *reinterpret_cast<const f4*>(&s_a0[i0]);  // one 16-byte LDS read covers the four rows
              const f4 aN = *reinterpret_cast<const f4*>(&s_aN[i0]);
              Kr[0] = ns_divided_difference(a0.x, a0j, aN.x, aNj, inv_2nrmR);
              Kr[1] = ns_divided_difference(a0.y, a0j, aN.y, aNj, inv_2nrmR);
              Kr[2] = ns_divided_difference(a0.z, a0j, aN.z, aNj, inv_2nrmR);
              Kr[3] = ns_divided_difference(a0.w, a0j, aN.w, aNj, inv_2nrmR);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int e = 4 * e4 + r, i = i0 + r;
              if (I < J || i <= j) {
                float v = 0.f;
                if (i < D && j < D) {
                  const float K = Kr[r];
                  const float cij = acc[n][e];
                  if (i == j) glam = fmaf(cij, -2.f * K * inv_lam2, glam);
                  v = cij * 0.5f * fmaf(s_beta[i] + bj, K, -1.f);
                }
                sY[i * LD + j] = v;
                sY[j * LD + i] = v;
              }
            }
          }
        }
      }
    }
    __syncthreads();
    KSTAMP(5);
    {
      // T2 = U (C o F)
      f32x16 acc[T::kPerWave];
      gemm_lds<NT, false, false, false>(sX, sY, acc);
      __syncthreads();
      store_tiles<NT>(sY, acc);
    }
    __syncthreads();
    KSTAMP(6);
    {
      // G_B = T2 U^T (symmetric: upper tiles) -> LDS ; G_out = GZ_direct - G_B ; dL/dlam -= <S, G_B>/lam^2
      f32x16 acc[TU::kPerWave];
      gemm_lds<NT, false, true, true>(sY, sX, acc);
      KSTAMP(7);
      __syncthreads();  // every wave is done reading sY / sX
#pragma unroll
      for (int n = 0; n < TU::kPerWave; ++n) {
        const int t = w + kWaves * n;
        if (t < TU::kCount) {
          int I, J;
          TU::ij(t, I, J);
#pragma unroll
          for (int e = 0; e < 16; ++e) sY[(I * 32 + acc_row(e, lane)) * LD + J * 32 + (lane & 31)] = acc[n][e];
        }
      }
    }
    __syncthreads();
    KSTAMP(20);
    {
      [[maybe_unused]] int p = p0, c = c0;
      for (int q0 = 0; q0 < kMaxQ; q0 += kQ) {
        // all reads of a pass first, then the writes: G_out goes into G_B's own buffer, and read / write / read / ... of one LDS array
        // is a chain of waits the compiler cannot reorder (19 k instead of 12 k ticks for this phase)
        int pk[kQ];
        float gb[kQ], sij[kQ];
#pragma unroll
        for (int u = 0; u < kQ; ++u) {
          if constexpr (kPre) {
            pk[u] = (int)(short)s_ent[u][tid];
          } else {
            pk[u] = (q0 + u < kMaxQ) ? entry(tid + kThreads * (q0 + u), p, c) : -1;
            advance(p, c);
          }
          const bool in = pk[u] >= 0;
          const int i = pk[u] >> kIShift, j = pk[u] & kJMask;
          gb[u] = sY[in ? i * LD + j : 0];  // (unconditional reads, clamped addresses: no branch per entry)
          // S_ij again from memory (L2: phase A read it this step) rather than 33 more registers held across the four products, which
          // spilled dL/dZ's direct part (21 VGPRs, reloaded one round trip at a time right here: 8 k ticks)
          // (a 32-bit offset: all of a pass's requests are issued before the first is waited for -- formed as Sm[i * D + j] with a 64-bit
          // multiply-add, every one of them was followed by an s_waitcnt vmcnt(0), one round trip per entry)
          sij[u] = load_at<float>(Sm, in ? 4u * ((unsigned)i * (unsigned)D + (unsigned)j) : 0u);
        }
        if (kPre) {
          // branch-free: an entry that does not exist writes to the padding column (never read) and adds zero -- with a branch per entry the
          // compiler loses count of the LDS operations in flight and waits for all of them before every pair of writes
#pragma unroll
          for (int u = 0; u < kQ; ++u) {
            const bool in = pk[u] >= 0;
            const int i = pk[u] >> kIShift, j = pk[u] & kJMask;
            const float o = gz[u] - gb[u];
            sY[in ? i * LD + j : DP] = o;  // in G_B's place: (i, j) is read by this thread alone, (j, i) by nobody (G_B lives on the upper triangle)
            sY[in ? j * LD + i : DP] = o;
            glam = fmaf(in ? -sij[u] * inv_lam2 * ((i == j) ? 1.f : 2.f) : 0.f, gb[u], glam);
          }
        } else {
#pragma unroll
          for (int u = 0; u < kQ; ++u) {
            if (pk[u] >= 0) {
              const int i = pk[u] >> kIShift, j = pk[u] & kJMask;
              const float o = Go[i * D + j] - gb[u];
              sY[i * LD + j] = o;
              sY[j * LD + i] = o;
              glam = fmaf(-sij[u] * inv_lam2 * ((i == j) ? 1.f : 2.f), gb[u], glam);
            }
          }
        }
#if UGLAD_CELL_BWD_GS
        {  // gS_ij += (G_B)_ij / lam_k, mirrored: only this thread touches gS_ij and gS_ji
          const float inv_lam = 1.0f / lam;
#pragma unroll
          for (int u = 0; u < kQ; ++u) {
            if (pk[u] >= 0) {
              const int i = pk[u] >> kIShift, j = pk[u] & kJMask;
              const float v = fmaf(gb[u], inv_lam, gS[base + i * D + j]);
              gS[base + i * D + j] = v;
              gS[base + j * D + i] = v;
            }
          }
        }
#endif
      }
    }
    __syncthreads();
    KSTAMP(21);
    if (last) {  // coalesced copy-out
      const int si = kThreads / D, sj = kThreads - si * D;
      int i = tid / D, j = tid - i * D;
      for (int idx = tid; idx < D * D; idx += kThreads) {
        Go[idx] = sY[i * LD + j];
        j += sj;
        i += si;
        if (j >= D) {
          j -= D;
          ++i;
        }
      }
    }
    KSTAMP(8);
    // ---- reductions: dL/dlam of this step; the 28 rhoNN gradients once, after the last step
    if (last) {
#pragma unroll
      for (int q = 0; q < kNRho; ++q) {
        if constexpr (kPackA) g[q] = g2[q].x + g2[q].y;
        const float v = wave_sum(g[q]);
        if (lane == 0) s_g[w][q] = v;
      }
    }
    {
      const float v = wave_sum(glam);
      if (lane == 0) s_g[w][kNRho] = v;
    }
    __syncthreads();
    if (tid == kNRho || (last && tid < kNRho)) {
      float v = 0.f;
#pragma unroll
      for (int ww = 0; ww < kWaves; ++ww) v += s_g[ww][tid];
      if (tid < kNRho)
        grad_rho_partial[(size_t)blockIdx.x * kNRho + tid] += v;
      else
        (glam_partial - (size_t)s * gridDim.x)[blockIdx.x] = v;
    }
    KSTAMP(9);
  }
}
