"""The fp64 attention oracle (ops/oracle64.py) and its tolerance are sound without a GPU, and have
teeth: an fp32 PyTorch emulation of the attention kernels' arithmetic (online softmax per key tile,
bf16 P into the P.V product, fp32 sums with the unrounded p in the denominator, the split ranges of
``item_range``, the merge of ``merge_state``, the 32x32 prefill kernel's deferred rescale) passes
``assert_within`` on the very inputs tests/test_attention_oracle_gpu.py feeds the HIP kernels, and
each deliberately wrong variant of it lies more than 4 tolerances outside on a named case. The
emulation follows the kernels' formulas, not their wave layout."""
import math

import pytest
import torch

from theroundtaible_amd import ops
from theroundtaible_amd.ops import oracle64 as o64
from theroundtaible_amd.ops import reference as ref

BF = torch.bfloat16
NEG = float("-inf")
RESCALE_LOG2 = 8.0                       # csrc/attention_prefill32.hip
LOG2E = torch.tensor(1.4426950408889634, dtype=torch.float32)


# ---- the emulation ------------------------------------------------------------------------------

def merge_state(M, L, O, m2, l2, o2):
    """csrc/attn_core.h merge_state, elementwise: a state without a live key (l2 == 0) is skipped."""
    live = l2 > 0
    Mc = torch.maximum(M, torch.where(live, m2, torch.full_like(m2, NEG)))
    Ms = torch.where(Mc == NEG, torch.zeros_like(Mc), Mc)
    a = torch.exp2(M - Ms)
    f = torch.where(live, torch.exp2(torch.where(live, m2, Ms) - Ms), torch.zeros_like(Ms))
    return Mc, L * a + f * l2, O * a[..., None] + f[..., None] * o2


def empty_state(R, hkv, G, d):
    return (torch.full((R, hkv, G), NEG), torch.zeros(R, hkv, G), torch.zeros(R, hkv, G, d))


def emu_tiles(qf, k, v, lim, tiles, sl2, defer=False, no_rescale=False):
    """Online softmax of rows ``qf`` [R, hkv, G, d] over the key tiles ``tiles`` = (first key, end
    key, first V row) of ``k`` / ``v`` [N, hkv, d]; row i sees the keys below ``lim[i]``."""
    R, hkv, G, d = qf.shape
    m, l, O = empty_state(R, hkv, G, d)
    for lo, hi, vlo in tiles:
        s = torch.einsum("rhgd,nhd->rhgn", qf, k[lo:hi]) * sl2
        hidden = torch.arange(lo, hi)[None, :] >= lim[:, None]
        s = s.masked_fill(hidden[:, None, None, :], NEG)
        tmax = s.amax(-1)
        mnew = torch.maximum(m, tmax)
        if defer:                        # the running max moves only past the slack
            mnew = torch.where(tmax > m + RESCALE_LOG2, mnew, m)
        mref = torch.where(mnew == NEG, torch.zeros_like(mnew), mnew)
        alpha = torch.exp2(m - mref)
        p = torch.exp2(s - mref[..., None])
        l = l * alpha + p.sum(-1)
        pv = torch.einsum("rhgn,nhd->rhgd", p.to(BF).float(), v[vlo:vlo + hi - lo])
        O = (O if no_rescale else O * alpha[..., None]) + pv
        m = mnew
    return m, l, O


def finish(L, O):
    inv = torch.where(L > 0, 1.0 / L, torch.zeros_like(L))
    return (O * inv[..., None]).to(BF)


def gather_row(case, s):
    """K, V of every entry of block-table row ``s`` (the padding entries too), fp32."""
    n = case.block_tables.shape[1] * o64.ATTN_BS
    k, v = o64._attn_gather(case.k_cache, case.v_cache, case.block_tables[s], n)
    return k.float(), v.float()


def split_ranges(ctx, b, b0, n, sh, splits):
    """csrc/attn_core.h item_range for every slot of sequence b's group: per slot the shared chunk
    (tiles every member's columns see) and, for b's own slots, the private split."""
    bs = o64.ATTN_BS
    mi, nslots, ntiles = b - b0, n * splits, (ctx + bs - 1) // bs
    sh_per = (sh + nslots - 1) // nslots
    npr = max(0, ntiles - sh)
    pr_per = (npr + splits - 1) // splits
    out = []
    for slot in range(nslots):
        m2, y = divmod(slot, splits)
        sh_b = min(sh, slot * sh_per)
        tiles = list(range(sh_b, min(sh, sh_b + sh_per)))
        if m2 == mi:
            tiles += list(range(sh + min(npr, y * pr_per), sh + min(npr, y * pr_per + pr_per)))
        out.append(tiles)
    return out


def emu_decode(case, splits, mutant=None):
    """The decode kernels' arithmetic (groups from ops.decode_groups as the launch gets them)."""
    bs, hq, hkv, d = o64.ATTN_BS, case.hq, case.hkv, case.d
    G = hq // hkv
    sl2 = torch.tensor(case.scale, dtype=torch.float32) * LOG2E
    groups, _ = ops.decode_groups(case.group_of, case.shared, G)
    out = torch.empty_like(case.q)
    for b in range(case.q.shape[0]):
        ctx = int(case.ctx_lens[b])
        b0, n, sh = (int(x) for x in groups[b])
        k, v = gather_row(case, b)
        qf = case.q[b].float().reshape(1, hkv, G, d)
        lim = torch.tensor([ctx - 1 if mutant == "last_key" else ctx + 1 if mutant == "poison" else ctx])
        M, L, O = empty_state(1, hkv, G, d)
        hit = False
        for tiles in split_ranges(ctx, b, b0, n, sh, splits):
            tl = [(t * bs, t * bs + bs, t * bs) for t in tiles]
            boundary = tiles and tiles[0] > 0 and not hit       # a slot that starts inside the row
            if mutant == "skip_tile" and boundary:
                tl, hit = tl[1:], True
            if mutant == "dup_tile" and boundary:
                tl, hit = tl[:1] + tl, True
            if mutant == "v_next" and tiles and tiles[0] == 0:
                tl[0] = (0, bs, bs)
            st = emu_tiles(qf, k, v, lim, tl, sl2, no_rescale=mutant == "no_rescale")
            M, L, O = merge_state(M, L, O, *st)
        out[b] = finish(L, O).reshape(hq, d)
    return out


def emu_prefill(case, plan=None, mutant=None):
    """The prefill kernels' arithmetic: 64-key tiles and the deferred rescale where the 32x32 kernel
    runs, 32-key tiles where the 16x16 one does; ``plan`` = ops.prefill_split_plan's (items, cmap,
    parts): each row tile's key-tile ranges leave partial states merged in part order."""
    hq, hkv, d = case.hq, case.hkv, case.d
    G = hq // hkv
    k32 = d == 128 and G <= 8
    kt = 64 if k32 else 32
    sl2 = torch.tensor(case.scale, dtype=torch.float32) * LOG2E
    out = torch.empty_like(case.q)
    parts = {}
    if plan is not None:
        for s, row0, tb, te, _ in sorted(plan[0].tolist(), key=lambda it: (it[0], it[1], it[2])):
            parts.setdefault((s, row0), []).append((tb, te))
    rows_per = o64.attn_prefill_rows(G, d)
    add = {"causal_lt": 0, "causal_le1": 2}.get(mutant, 1)
    for s, (st, new) in enumerate(case.specs):
        a = int(case.cu_q[s])
        k, v = gather_row(case, s)
        for row0 in (range(a, a + new, rows_per) if plan is not None else [a]):
            row1 = min(a + new, row0 + rows_per) if plan is not None else a + new
            qf = case.q[row0:row1].float().reshape(row1 - row0, hkv, G, d)
            pos = st + torch.arange(row0 - a, row1 - a)
            kmax = st + row1 - a
            nkt = (kmax + kt - 1) // kt
            M, L, O = empty_state(row1 - row0, hkv, G, d)
            for tb, te in parts.get((s, row0), [(0, nkt)]):
                # keys of the last tile past the rows' reach are hidden by the causal limit alone
                tl = [(t * kt, min(t * kt + kt, k.shape[0]), t * kt) for t in range(tb, min(te, nkt))]
                M, L, O = merge_state(M, L, O, *emu_tiles(qf, k, v, pos + add, tl, sl2, defer=k32))
            out[row0:row1] = finish(L, O).reshape(row1 - row0, hq, d)
    return out


def split_plan(case, min_chunk):
    rows = o64.attn_prefill_rows(case.hq // case.hkv, case.d)
    plan = ops.prefill_split_plan(case.cu_q, rows, case.start_pos, case.hkv, num_cus=1 << 20,
                                  min_chunk_tiles=min_chunk)
    assert plan is not None and plan[2] >= 2
    return plan


def ref32(case, prefill):
    """The fp32 CPU reference's output before its bf16 cast."""
    if prefill:
        return ref.prefill_attention(case.q.float(), case.k_cache, case.v_cache, case.block_tables, case.cu_q,
                                     case.start_pos, case.scale)
    return ref.paged_attention_decode(case.q.float(), case.k_cache, case.v_cache, case.block_tables, case.ctx_lens,
                                      case.scale)


REF_WORST = {}


def note_reference(name, case, e, A, prefill):
    """|o32 - e| / A of the fp32 reference on this case (the figure ATTN_SLACK is 4x of), and the
    reference itself inside the tolerance."""
    o32 = ref32(case, prefill).double()
    err = (o32 - e).abs()
    assert bool((err[A == 0] == 0).all()), name
    REF_WORST[name] = float((err / A.clamp_min(1e-300))[A > 0].max())
    o64.assert_within(o32.float().to(BF), e, o64.attn_tol(e, A, case.p_exact), name + " reference")


# ---- soundness: the emulation inside the bound on every builder case of the GPU test --------------

@pytest.mark.parametrize("kind", o64.ATTN_KINDS)
@pytest.mark.parametrize("cfg", o64.ATTN_DECODE_CFGS)
def test_decode_emulation_within_bound(cfg, kind):
    case = o64.attn_decode_case(kind, *cfg)
    e, A, tol = o64.attn_oracle(case)
    note_reference(f"decode {cfg} {kind}", case, e, A, False)
    for splits in o64.ATTN_DECODE_SPLITS:
        r = o64.assert_within(emu_decode(case, splits), e, tol, f"decode {cfg} {kind} splits {splits}")
        print(f"decode {cfg} {kind} splits {splits}: error / tolerance {r:.3f}")


@pytest.mark.parametrize("kind", o64.ATTN_REFILL_KINDS)
def test_decode_refill_emulation_within_bound(kind):
    cfg = o64.ATTN_REFILL_CFGS[0]
    case = o64.attn_decode_case(kind, *cfg, lens=o64.ATTN_REFILL_LENS)
    e, A, tol = o64.attn_oracle(case)
    note_reference(f"refill {cfg} {kind}", case, e, A, False)
    for splits in o64.ATTN_REFILL_SPLITS:
        o64.assert_within(emu_decode(case, splits), e, tol, f"refill {cfg} {kind} splits {splits}")


@pytest.mark.parametrize("kind", o64.ATTN_KINDS)
@pytest.mark.parametrize("cfg", o64.ATTN_GROUP_CFGS)
def test_grouped_decode_emulation_within_bound(cfg, kind):
    case = o64.attn_group_case(kind, *cfg)
    e, A, tol = o64.attn_oracle(case)
    note_reference(f"grouped {cfg} {kind}", case, e, A, False)
    for splits in o64.ATTN_GROUP_SPLITS:
        o64.assert_within(emu_decode(case, splits), e, tol, f"grouped {cfg} {kind} splits {splits}")


@pytest.mark.parametrize("kind", o64.ATTN_KINDS)
@pytest.mark.parametrize("cfg", o64.ATTN_PREFILL_CFGS)
def test_prefill_emulation_within_bound(cfg, kind):
    case = o64.attn_case(kind, *cfg, o64.ATTN_PREFILL_SPECS)
    e, A, tol = o64.attn_oracle(case, prefill=True)
    note_reference(f"prefill {cfg} {kind}", case, e, A, True)
    r = o64.assert_within(emu_prefill(case), e, tol, f"prefill {cfg} {kind}")
    print(f"prefill {cfg} {kind}: error / tolerance {r:.3f}")


@pytest.mark.parametrize("kind", o64.ATTN_KINDS)
@pytest.mark.parametrize("cfg", o64.ATTN_SPLIT_CFGS)
def test_prefill_key_split_emulation_within_bound(cfg, kind):
    case = o64.attn_case(kind, *cfg, o64.ATTN_SPLIT_SPECS)
    e, A, tol = o64.attn_oracle(case, prefill=True)
    note_reference(f"key split {cfg} {kind}", case, e, A, True)
    o64.assert_within(emu_prefill(case), e, tol, f"key split {cfg} {kind} whole")
    for mc in o64.ATTN_SPLIT_MIN_CHUNK:
        o64.assert_within(emu_prefill(case, split_plan(case, mc)), e, tol, f"key split {cfg} {kind} chunk {mc}")


def every_case():
    """(name, builder, prefill) of every case of the lists above, named as note_reference names them."""
    for kind in o64.ATTN_KINDS:
        for cfg in o64.ATTN_DECODE_CFGS:
            yield f"decode {cfg} {kind}", (lambda c=cfg, k=kind: o64.attn_decode_case(k, *c)), False
        for cfg in o64.ATTN_GROUP_CFGS:
            yield f"grouped {cfg} {kind}", (lambda c=cfg, k=kind: o64.attn_group_case(k, *c)), False
        for cfg in o64.ATTN_PREFILL_CFGS:
            yield f"prefill {cfg} {kind}", (lambda c=cfg, k=kind: o64.attn_case(k, *c, o64.ATTN_PREFILL_SPECS)), True
        for cfg in o64.ATTN_SPLIT_CFGS:
            yield f"key split {cfg} {kind}", (lambda c=cfg, k=kind: o64.attn_case(k, *c, o64.ATTN_SPLIT_SPECS)), True
    for kind in o64.ATTN_REFILL_KINDS:
        cfg = o64.ATTN_REFILL_CFGS[0]
        yield (f"refill {cfg} {kind}", (lambda c=cfg, k=kind: o64.attn_decode_case(k, *c, lens=o64.ATTN_REFILL_LENS)),
               False)


def test_reference_worst_is_recorded():
    """ATTN_REF_WORST bounds the fp32 reference's worst |o32 - e| / A over every case above (noted by
    the soundness tests when they ran before this one, computed here otherwise), and ATTN_SLACK is
    4x it rounded up to a power of two."""
    for name, build, prefill in every_case():
        if name not in REF_WORST:
            case = build()
            e, A, _ = o64.attn_oracle(case, prefill)
            note_reference(name, case, e, A, prefill)
    name, worst = max(REF_WORST.items(), key=lambda kv: kv[1])
    print(f"ATTN_REF_WORST measured {worst:.4g} at {name}; recorded {o64.ATTN_REF_WORST:.4g}")
    assert worst <= o64.ATTN_REF_WORST
    assert o64.ATTN_SLACK == 2.0 ** math.ceil(math.log2(4 * o64.ATTN_REF_WORST))


def test_split_ranges_cover_every_tile_once():
    """The emulation's item ranges: every tile of a row exactly once over its slots."""
    for ctx, n, sh, splits in ((1500, 1, 0, 64), (460, 3, 5, 10), (96, 4, 3, 8), (2420, 2, 60, 3), (33, 1, 0, 3)):
        for mi in range(n):
            seen = sorted(t for tl in split_ranges(ctx, mi, 0, n, sh, splits) for t in tl)
            assert seen == list(range((ctx + 31) // 32)), (ctx, n, sh, splits, mi)


# ---- teeth: wrong emulations exceed error / tolerance 4 on a named case -----------------------------

DECODE_MUTANTS = {
    # mutant: (kind, config, splits) of the case that catches it
    "last_key": ("census", (32, 8, 128), 3),      # the last live key is masked
    "poison": ("random", (32, 8, 128), 1),        # the first key past ctx_len is admitted
    "skip_tile": ("census", (8, 1, 128), 3),      # one tile at a split boundary is skipped
    "dup_tile": ("census", (8, 1, 128), 3),       # one tile is read twice
    "no_rescale": ("ramp_r8", (28, 4, 128), 1),   # the O rescale is skipped when the max moves
    "v_next": ("census", (12, 12, 64), 8),        # one tile's V comes from the next block-table entry
}


@pytest.mark.parametrize("mutant", sorted(DECODE_MUTANTS))
def test_decode_mutant_is_caught(mutant):
    kind, cfg, splits = DECODE_MUTANTS[mutant]
    case = o64.attn_decode_case(kind, *cfg)
    e, A, tol = o64.attn_oracle(case)
    o64.assert_within(emu_decode(case, splits), e, tol, "unmutated")
    r = o64.error_ratio(emu_decode(case, splits, mutant), e, tol)
    print(f"{mutant} on decode {cfg} {kind} splits {splits}: error / tolerance {r:.1f}")
    assert r > 4.0


@pytest.mark.parametrize("mutant", sorted(DECODE_MUTANTS))
def test_decode_mutant_is_caught_on_short_random_rows(mutant):
    """Each also on the plain random rows (1..257 keys; 1500 for the tile mutants' split ranges)."""
    case = o64.attn_decode_case("random", 32, 8, 128)
    e, A, tol = o64.attn_oracle(case)
    r = o64.error_ratio(emu_decode(case, 3, mutant), e, tol)
    print(f"{mutant} on decode random splits 3: error / tolerance {r:.1f}")
    assert r > 4.0


PREFILL_MUTANTS = {"causal_lt": ("census", (32, 8, 128)),      # key < pos
                   "causal_le1": ("ramp_r8", (12, 12, 64))}    # key <= pos + 1


@pytest.mark.parametrize("mutant", sorted(PREFILL_MUTANTS))
def test_prefill_mutant_is_caught(mutant):
    kind, cfg = PREFILL_MUTANTS[mutant]
    case = o64.attn_case(kind, *cfg, o64.ATTN_PREFILL_SPECS)
    e, A, tol = o64.attn_oracle(case, prefill=True)
    r = o64.error_ratio(emu_prefill(case, mutant=mutant), e, tol)
    print(f"{mutant} on prefill {cfg} {kind}: error / tolerance {r:.1f}")
    assert r > 4.0
    rr = o64.error_ratio(emu_prefill(o64.attn_case("random", *cfg, o64.ATTN_PREFILL_SPECS), mutant=mutant),
                         *o64.attn_oracle(o64.attn_case("random", *cfg, o64.ATTN_PREFILL_SPECS), prefill=True)[::2])
    print(f"{mutant} on prefill {cfg} random: error / tolerance {rr:.1f}")
    assert rr > 4.0


def test_poison_layout():
    """Padding entries point to one dedicated block nobody's live range uses; every slot past a row's
    end, every unreferenced block and the dedicated block hold V = 96 and finite K."""
    case = o64.attn_group_case("random", 32, 8, 128)
    bt, bs = case.block_tables, o64.ATTN_BS
    live = set()
    for s, n in enumerate(case.ctx_lens.tolist()):
        nblk = (n + bs - 1) // bs
        live |= set(bt[s, :nblk].tolist())
        assert bool((bt[s, nblk:] == case.poison_block).all())
        tail = case.v_cache[int(bt[s, nblk - 1])][:, :, n - (nblk - 1) * bs:]
        assert bool((tail == o64.ATTN_POISON_V).all())
    assert case.poison_block not in live
    dead = [b for b in range(case.k_cache.shape[0]) if b not in live]
    assert len(dead) == 4 and bool((case.v_cache[dead] == o64.ATTN_POISON_V).all())
    assert bool(torch.isfinite(case.k_cache.float()).all()) and bool((case.k_cache[dead].float().abs().amax() > 0))
