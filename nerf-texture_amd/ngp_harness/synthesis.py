"""The middle step of the texture pipeline: a large planar feature map synthesized from exported patches, on the device.

The reference does this offline on the CPU (patch_matching_and_quilting.py: class patchBasedTextureSynthesis and the options under __main__) and
writes texture.npz; `synthesize_texture` takes what `CurvedField.export_field` returns and gives the arrays `CurvedField.import_field` takes.
The kernels and the contract: csrc/synthesis.inc, include/nerftex_hip.h (nerftex_synth_*).  Built: mode 'Cut', no quilting, the coarse strips,
no rotation, the close-patch filter over picked_vertices, both mirrors and strict_match selectable.  Refused: mode='blend', quilt=True, an export
without picked_vertices (the reference's checkForMirrors filter) and a non-square output.
"""
import ctypes
import math

import numpy as np

REFUSED = {"mode": "only mode='Cut' is built (mode='blend' is refused)", "quilt": "quilt=True is refused (the reference's script runs without quilting)"}


class SynthesisExhausted(RuntimeError):
    """The close-patch filter removed every candidate of a cell and the next k exceeds the example set (sklearn raises at the same point)."""


def default_sizes(S):
    """The script's sizes for S-pixel patches (:471-480): patchSize = int(S / 4), one less if S - patchSize is odd; overlapSize the rest halved."""
    ps = int(S / 4)
    if (S - ps) % 2 == 1:
        ps -= 1
    return ps, (S - ps) // 2


def canvas_cells(output_size, patch_size, overlap_size):
    """initCanvas (:319): -> (cells per side, canvas side)."""
    n = int(math.ceil((output_size - overlap_size) / (patch_size + overlap_size)))
    return n, n * patch_size + (n + 1) * overlap_size


def _output_side(output_size):
    if isinstance(output_size, (tuple, list, np.ndarray)):
        if len(output_size) != 2 or int(output_size[0]) != int(output_size[1]):
            raise NotImplementedError(f"synthesize_texture: a non-square output {tuple(output_size)} is refused")
        return int(output_size[0])
    return int(output_size)


def synthesize_texture(result, output_size, *, patch_size=None, overlap_size=None, mirror_hor=False, mirror_vert=False, strict_match=True, close_threshold=0.2,
                       max_patch_res=32, first_patch=None, draws=None, seed=None, forced=None, light_maps=None, mode="Cut", quilt=False, device=None):
    """result: what `export_field` returns -- `patches` [P,S,S,F], `grid_gap`, `patch_sample_tbn` [P,9], `picked_vertices` [P,3], and
    `patch_phi_embed` [P,S,S,8] / `patch_local_tbn` [P,S,S,9] or None.  The features are what is matched (match_dim = F); phi_embed and local_tbn
    ride along as further channels.  output_size: the side of the square map asked for (or a pair of equal sides); the map returned is the next
    size that holds whole cells (`canvas_cells`).
      patch_size, overlap_size   default: the script's (`default_sizes`); overlap_size * 2 + patch_size must be S
      strict_match               attenuation 3 (True) or 1
      first_patch                the example of cell (0, 0), < examples; default: drawn from `seed` (the reference's randint can pick one past the end)
      draws                      one uniform number in [0, 1) per cell behind the first; default np.random.RandomState(seed).random_sample(cells - 1)
      forced                     [cells] ids to place instead of the drawn ones (entry 0 is ignored); what the draw picks is still logged
      light_maps                 whether the texture carries the four maps of a lit field; default: the export has patch_phi_embed
    -> (texture, log).  texture: `features` [H,W,F], `grid_gap`, `phi_embed`, `local_tbn`, `sample_tbn` [n,9], `sample_tbn_ids` [H,W] -- device
    tensors, so that `field.import_field(**texture)` works; the last four are None without light maps (import_field takes all four or none).
    log: `id_map` [n,n], `canvas_id` [H,W] (example ids), `total_id`, `sample_tbn`, `sample_tbn_ids`, and per cell `k`, `survivor_count`, `drawn`,
    `placed`, `ranked_ids` [cells,16], `survivors` [cells,16] (-1 padded), `ranked_dist` [cells,16] float64, plus `draws` and `first_patch`."""
    import torch

    from nerftex_hip import ERR_EXHAUSTED, SYNTH_BLEND, SYNTH_CANVAS, SYNTH_CANVAS_ID, SYNTH_CUT, SYNTH_ID_MAP, SYNTH_LOG_DIST, SYNTH_LOG_IDS, SYNTH_LOG_STRIDE, \
        SYNTH_TBN, SYNTH_TBN_IDS, SYNTH_TOTAL_ID, SynthDesc, SynthView, check, lib, ptr, stream

    if mode not in ("Cut", "blend"):
        raise ValueError(f"synthesize_texture: mode is 'Cut' or 'blend', not {mode!r}")
    if mode != "Cut":
        raise NotImplementedError("synthesize_texture: " + REFUSED["mode"])
    if quilt:
        raise NotImplementedError("synthesize_texture: " + REFUSED["quilt"])
    if result.get("picked_vertices") is None:
        raise NotImplementedError("synthesize_texture: picked_vertices are required (the picked_vertices=None neighbour filter, checkForMirrors, is refused)")
    side_asked = _output_side(output_size)
    dev = torch.device("cuda" if device is None else device)

    def on_device(a):
        return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(device=dev, dtype=torch.float32)

    feats = on_device(result["patches"])
    if feats.dim() != 4 or feats.shape[1] != feats.shape[2] or feats.shape[0] < 1:
        raise ValueError(f"synthesize_texture: patches are [P, S, S, F], but got {tuple(feats.shape)}")
    P, S, F = int(feats.shape[0]), int(feats.shape[1]), int(feats.shape[3])
    phi, loc = result.get("patch_phi_embed"), result.get("patch_local_tbn")
    parts, n_phi = [feats], 0
    if phi is not None:
        parts.append(on_device(phi).reshape(P, S, S, -1))
        n_phi = int(parts[-1].shape[-1])
    if loc is not None:
        parts.append(on_device(loc).reshape(P, S, S, 9))
    patches = torch.cat(parts, dim=-1).contiguous() if len(parts) > 1 else feats.contiguous()
    C = int(patches.shape[-1])
    sample_tbn = on_device(result["patch_sample_tbn"]).reshape(P, 9).contiguous()
    picked = on_device(result["picked_vertices"]).reshape(P, 3).contiguous()
    grid_gap = float(result["grid_gap"])
    ps0, _ = default_sizes(S)
    ps = ps0 if patch_size is None else int(patch_size)
    ov = (S - ps) // 2 if overlap_size is None else int(overlap_size)
    examples = P * (2 if mirror_hor else 1) * (2 if mirror_vert else 1)

    desc = SynthDesc(patches=ptr(patches), sample_tbn=ptr(sample_tbn), picked_vertices=ptr(picked), P=P, S=S, C=C, match_dim=F, patch_size=max(ps, 0),
                     overlap_size=max(ov, 0), output_h=side_asked, output_w=side_asked, mirror_hor=int(bool(mirror_hor)), mirror_vert=int(bool(mirror_vert)),
                     attenuation=3 if strict_match else 1, max_patch_res=int(max_patch_res), mode=SYNTH_CUT if mode == "Cut" else SYNTH_BLEND, quilt=int(bool(quilt)),
                     close_threshold=float(close_threshold), patch_length=S * grid_gap)
    handle = ctypes.c_void_p()
    torch.cuda.current_stream(dev).synchronize()  # create works on the default stream
    with torch.cuda.device(dev):
        check(lib.nerftex_synth_create(ctypes.byref(desc), ctypes.byref(handle)))
        try:
            view = SynthView()
            check(lib.nerftex_synth_result(handle, ctypes.byref(view)))
            n, side, cells = int(view.cells_per_side), int(view.side), int(view.cells_per_side) ** 2
            rng = np.random.RandomState(seed)
            if first_patch is None:
                first_patch = int(np.random.RandomState(seed).randint(0, examples)) if seed is not None else int(np.random.randint(0, examples))
            if not 0 <= int(first_patch) < examples:
                raise ValueError(f"synthesize_texture: first_patch {first_patch} is outside the {examples} examples")
            draws = rng.random_sample(cells - 1) if draws is None else np.asarray(draws, dtype=np.float64).reshape(-1)
            if draws.shape[0] != cells - 1:
                raise ValueError(f"synthesize_texture: {cells - 1} draws are needed (one per cell behind the first), but got {draws.shape[0]}")
            draws_dev = torch.from_numpy(np.concatenate([[0.0], draws])).to(dev)
            forced_dev = None
            if forced is not None:
                forced = np.asarray(forced, dtype=np.int64).reshape(-1)
                if forced.shape[0] != cells:
                    raise ValueError(f"synthesize_texture: forced holds one id per cell ({cells}), but got {forced.shape[0]}")
                forced_dev = torch.from_numpy(forced.astype(np.int32)).to(dev)
            st = stream()
            check(lib.nerftex_synth_resolve(handle, int(first_patch), ptr(draws_dev), ptr(forced_dev), 0, cells, st))
            rc = lib.nerftex_synth_finish(handle, st)
            if rc == ERR_EXHAUSTED:
                raise SynthesisExhausted(lib.nerftex_last_error().decode())
            check(rc)
            check(lib.nerftex_synth_result(handle, ctypes.byref(view)))
            n_total = int(view.n_total)

            def read(what, shape, dtype):
                t = torch.empty(shape, dtype=dtype, device=dev)
                if t.numel():
                    check(lib.nerftex_synth_read(handle, what, ptr(t), t.numel() * t.element_size(), st))
                return t

            canvas = read(SYNTH_CANVAS, (side, side, C), torch.float32)
            canvas_id = read(SYNTH_CANVAS_ID, (side, side), torch.int32)
            id_map = read(SYNTH_ID_MAP, (n, n), torch.int32)
            log_ids = read(SYNTH_LOG_IDS, (cells, SYNTH_LOG_STRIDE), torch.int32)
            log_dist = read(SYNTH_LOG_DIST, (cells, 16), torch.float64)
            tbn_ids = read(SYNTH_TBN_IDS, (side, side), torch.int32)
            tbn = read(SYNTH_TBN, (n_total, 9), torch.float32)
            total_id = read(SYNTH_TOTAL_ID, (n_total,), torch.int32)
            torch.cuda.current_stream(dev).synchronize()
        finally:
            check(lib.nerftex_synth_destroy(handle))
    lit = (phi is not None) if light_maps is None else bool(light_maps)
    if lit and (phi is None or loc is None):
        raise ValueError("synthesize_texture: light_maps needs an export with patch_phi_embed and patch_local_tbn")
    texture = {
        "features": canvas[..., :F].contiguous(),
        "grid_gap": grid_gap,
        "phi_embed": canvas[..., F:F + n_phi].contiguous() if lit else None,
        "local_tbn": canvas[..., C - 9:].contiguous() if lit else None,
        "sample_tbn": tbn if lit else None,
        "sample_tbn_ids": tbn_ids if lit else None,
    }
    li = log_ids.cpu().numpy()
    log = {"id_map": id_map.cpu().numpy(), "canvas_id": canvas_id.cpu().numpy(), "total_id": total_id.cpu().numpy(), "sample_tbn": tbn.cpu().numpy(),
           "sample_tbn_ids": tbn_ids.cpu().numpy(), "k": li[:, 0], "survivor_count": li[:, 1], "drawn": li[:, 2], "placed": li[:, 3], "ranked_ids": li[:, 4:20],
           "survivors": li[:, 20:36], "ranked_dist": log_dist.cpu().numpy(), "draws": draws, "first_patch": int(first_patch), "canvas": canvas,
           "cells_per_side": n, "patch_size": ps, "overlap_size": ov, "examples": examples, "block": int(view.block), "strip_floats": int(view.strip_floats)}
    return texture, log
