"""Stage-1 (pre-training) forward shared by ISD (model_2D.py:215-305) and ISD_3d (model_3D.py:309-403): student and
momentum-teacher passes through the HIP U-Net / V-Net, latent and patch-wise output embeddings compared with two queues.
The heads are a few 2- to 256-wide layers on pooled maps and run as plain tensor ops around the two networks."""
import torch
import torch.nn as nn
import torch.nn.functional as F


def get_shuffle_ids(bsz, device=None):
    """ShuffleBN permutation and its inverse (model_2D.py:308-318).  Drawn from the torch CPU generator, like the
    reference's torch.randperm(bsz).long().cuda()."""
    forward_inds = torch.randperm(bsz).long()
    backward_inds = torch.zeros(bsz).long()
    backward_inds.index_copy_(0, forward_inds, torch.arange(bsz).long())
    return forward_inds.to(device), backward_inds.to(device)


def compute_logits(z_anchor, z_positive, temp_fac):
    """Cosine similarities of every anchor row with every queue row over the temperature (model_2D.py:320-331)."""
    z_anchor = nn.functional.normalize(z_anchor, dim=1)
    z_positive = nn.functional.normalize(z_positive, dim=1)
    return torch.matmul(z_anchor, z_positive.T) / temp_fac


def dequeue_and_enqueue(K, keys, queue, queue_ptr):
    """model_2D.py:201-212: keys overwrite queue[ptr : ptr + batch], the pointer wraps at K."""
    batch_size = keys.shape[0]
    ptr = int(queue_ptr)
    assert K % batch_size == 0
    queue[ptr:ptr + batch_size] = keys
    queue_ptr[0] = (ptr + batch_size) % K


def _unwrap(m):
    return m.module if hasattr(m, "module") else m


def _pool_size(pool_layer):
    o = pool_layer.output_size
    return o if isinstance(o, int) else o[0]


class PatchPoolFn(torch.autograd.Function):
    """adaptive_avg_pool{2,3}d(., pool) of every patch of the patch / 2-stride grid of x [B, C, n...] as one kernel each way
    (csrc/patch_pool.hip): [P, B, C, pool...], patch number first, the layout torch.cat of the per-patch results has.  Linear, so
    the backward needs the geometry alone: no tensor is saved."""

    @staticmethod
    def forward(ctx, x, patch, pool):
        from . import _lib as L
        L.require_gpu(x)
        if x.dtype != torch.float32 or x.dim() not in (4, 5):
            raise ValueError(f"PatchPoolFn: an fp32 [B, C, n...] map with 2 or 3 spatial axes, got {x.dtype} {tuple(x.shape)}")
        x = x.contiguous()
        nd, n = x.dim() - 2, tuple(x.shape[2:])
        step = max(int(patch) // 2, 1)
        P = 1
        for s in n:
            P *= max((s - patch) // step + 1, 0)          # 0: no patch fits; the entry point refuses the empty output
        y = torch.empty((P, x.shape[0], x.shape[1]) + (int(pool),) * nd, dtype=torch.float32, device=x.device)
        ctx.geom = (nd, x.shape[0], x.shape[1]) + n + (1,) * (3 - nd) + (int(patch), int(pool))
        L.call("arco_patch_pool_fwd", L.ptr(x), *ctx.geom, L.ptr(y))
        return y

    @staticmethod
    def backward(ctx, gy):
        from . import _lib as L
        nd, B, C = ctx.geom[:3]
        gy = gy.contiguous()
        gx = torch.empty((B, C) + tuple(ctx.geom[3:3 + nd]), dtype=torch.float32, device=gy.device)
        L.call("arco_patch_pool_bwd", L.ptr(gy), *ctx.geom, L.ptr(gx))
        return gx, None, None


FUSED_MAX_LAYERS, FUSED_MAX_WIDTH = 4, 32          # csrc/patch_head.hip PH_MAX_LAYERS, PH_MAX_WIDTH


class PatchHeadFn(torch.autograd.Function):
    """PatchPoolFn followed by 1 to 4 pointwise layers (kernel-1 convolutions, no non-linearity between them) as one kernel each way
    (csrc/patch_head.hip): x [B, C, n...] -> [P * B, C_out, pool...], the stacked tensor of patch_heads(route="gpu").  params is
    (weight, bias or None) per layer, flattened.  The pooled tensor [P, B, C, pool...] is saved; the backward computes the layers'
    activations again from it, sums the parameter gradients in float64 and runs PatchPoolFn's backward kernel on the gradient of the
    pooled tensor - unless x needs no gradient (the teacher's map), which skips both that kernel and the tensor."""

    @staticmethod
    def forward(ctx, x, patch, pool, *params):
        from . import _lib as L
        L.require_gpu(x, *params)
        if x.dtype != torch.float32 or x.dim() not in (4, 5):
            raise ValueError(f"PatchHeadFn: an fp32 [B, C, n...] map with 2 or 3 spatial axes, got {x.dtype} {tuple(x.shape)}")
        n_layers = len(params) // 2
        if len(params) % 2 or not 1 <= n_layers <= FUSED_MAX_LAYERS:
            raise ValueError(f"PatchHeadFn: 1 to {FUSED_MAX_LAYERS} (weight, bias) pairs, got {len(params)} tensors")
        x = x.contiguous()
        nd, n = x.dim() - 2, tuple(x.shape[2:])
        ws, bs, widths = [], [], [x.shape[1]]
        for k in range(n_layers):
            w, b = params[2 * k], params[2 * k + 1]
            if w.dtype != torch.float32 or w.dim() != nd + 2 or w.shape[1] != widths[-1] or tuple(w.shape[2:]) != (1,) * nd:
                raise ValueError(f"PatchHeadFn: layer {k} needs an fp32 weight [out, {widths[-1]}" + ", 1" * nd + f"], got {w.dtype} {tuple(w.shape)}")
            if b is not None and (b.dtype != torch.float32 or tuple(b.shape) != (w.shape[0],)):
                raise ValueError(f"PatchHeadFn: layer {k} needs an fp32 bias [{w.shape[0]}], got {b.dtype} {tuple(b.shape)}")
            ws.append(w.detach().contiguous())
            bs.append(None if b is None else b.detach().contiguous())
            widths.append(w.shape[0])
        if max(widths) > FUSED_MAX_WIDTH:
            raise ValueError(f"PatchHeadFn: widths up to {FUSED_MAX_WIDTH}, got {widths}")
        step = max(int(patch) // 2, 1)
        P = 1
        for s in n:
            P *= max((s - patch) // step + 1, 0)          # 0: no patch fits; the entry point refuses the empty output
        B, C = x.shape[0], x.shape[1]
        cells = (int(pool),) * nd
        pooled = torch.empty((P, B, C) + cells, dtype=torch.float32, device=x.device)
        y = torch.empty((P * B, widths[-1]) + cells, dtype=torch.float32, device=x.device)
        pad = FUSED_MAX_LAYERS - n_layers
        ctx.geom = (nd, B, C) + n + (1,) * (3 - nd) + (int(patch), int(pool))
        ctx.chain = (n_layers, tuple(widths[1:]) + (0,) * pad)
        L.call("arco_patch_head_fwd", L.ptr(x), *ctx.geom, n_layers, *_chain_ptrs(ws, bs, pad), *ctx.chain[1], L.ptr(pooled), L.ptr(y))
        ctx.has_bias = [b is not None for b in bs]
        ctx.save_for_backward(pooled, *ws, *[b for b in bs if b is not None])
        return y

    @staticmethod
    def backward(ctx, gy):
        from . import _lib as L
        nd, B, C = ctx.geom[:3]
        n_layers, widths = ctx.chain
        pad = FUSED_MAX_LAYERS - n_layers
        pooled, saved = ctx.saved_tensors[0], list(ctx.saved_tensors[1:])
        ws, rest = saved[:n_layers], saved[n_layers:]
        bs = [rest.pop(0) if hb else None for hb in ctx.has_bias]
        gy = gy.contiguous()
        need = ctx.needs_input_grad
        d0 = torch.empty_like(pooled) if need[0] else None
        n_bytes = L.query("arco_patch_head_ws_bytes", *ctx.geom, n_layers, *widths)
        if n_bytes <= 0:
            raise RuntimeError(f"arco_amd: arco_patch_head_ws_bytes refused {ctx.geom} {ctx.chain}")
        slabs = torch.empty(n_bytes // 8, dtype=torch.float64, device=gy.device)
        L.call("arco_patch_head_bwd", L.ptr(pooled), L.ptr(gy), *ctx.geom, n_layers, *_chain_ptrs(ws, bs, pad), *widths, L.ptr(d0), L.ptr(slabs))
        grads = []
        for k in range(n_layers):
            grads.append(torch.empty_like(ws[k]) if need[3 + 2 * k] else None)
            grads.append(torch.empty_like(bs[k]) if bs[k] is not None and need[4 + 2 * k] else None)
        if any(g is not None for g in grads):
            L.call("arco_patch_head_wgrad_finish", L.ptr(slabs), *ctx.geom, n_layers, *widths, *[L.ptr(g) for g in grads], *[None] * (2 * pad))
        gx = None
        if need[0]:
            gx = torch.empty((B, C) + tuple(ctx.geom[3:3 + nd]), dtype=torch.float32, device=gy.device)
            L.call("arco_patch_pool_bwd", L.ptr(d0), *ctx.geom, L.ptr(gx))
        return (gx, None, None) + tuple(grads)


def _chain_ptrs(ws, bs, pad):
    from . import _lib as L
    out = []
    for w, b in zip(ws, bs):
        out += [L.ptr(w), L.ptr(b)]
    return out + [None] * (2 * pad)


def _fused_params(layers, nd):
    """The (weight, bias) pairs of the layers for PatchHeadFn; ValueError, naming the limit, for a head the fused kernels do not take."""
    kind = nn.Conv2d if nd == 2 else nn.Conv3d
    if not 1 <= len(layers) <= FUSED_MAX_LAYERS:
        raise ValueError(f"patch_heads: the fused route takes 1 to {FUSED_MAX_LAYERS} pointwise layers, got {len(layers)}")
    params = []
    for l in layers:
        one = (1,) * nd
        if not (isinstance(l, kind) and tuple(l.kernel_size) == one and tuple(l.stride) == one and l.groups == 1
                and tuple(l.padding) == (0,) * nd):
            raise ValueError(f"patch_heads: the fused route takes kernel-1, stride-1, groups-1 {kind.__name__} layers without padding, got {l}")
        if max(l.in_channels, l.out_channels) > FUSED_MAX_WIDTH:
            raise ValueError(f"patch_heads: the fused route takes widths up to {FUSED_MAX_WIDTH}, got {l}")
        params += [l.weight, l.bias]
    return params


def patch_heads(x, patch, head, predictor, route="torch"):
    """predictor(head(x[..., i:i+p, j:j+p(, k:k+p)])) for every patch of the p/2-stride grid, in the reference's loop
    order (first spatial axis outermost; model_2D.py:263-268, model_3D.py:355-359).  The head is adaptive average pooling
    followed by 1x1 convolutions: when the pooling windows tile the patch stride, the pooled grid of the WHOLE map is
    computed once (avg_pool with the same windows), the pointwise layers run once on it, and a patch is a window of that
    grid - the same values, hundreds of small launches less (700 patches per volume in 3-D); otherwise the patches are
    taken one by one like the reference.
    route="gpu": one PatchPoolFn call pools every patch, whatever the patch and pooling sizes, the pointwise layers run once on the
    [P * B, C, pool...] tensor, and that STACKED tensor is returned (torch.cat of the list above, without the cat).
    route="fused": the same stacked tensor from one PatchHeadFn call, pooling and pointwise layers in one kernel each way
    (csrc/patch_head.hip); ValueError for a head it does not take (a layer that is not a kernel-1, stride-1, groups-1 convolution, more
    than 4 layers, a width above 32, a map that is not fp32) - no fallback to another route."""
    nd = x.dim() - 2
    conv = F.conv2d if nd == 2 else F.conv3d
    proj = _unwrap(head).proj
    pool_out = _pool_size(proj[0])
    layers = list(proj[1:]) + (list(_unwrap(predictor)) if predictor is not None else [])
    step = patch // 2
    starts = [range(0, x.shape[2 + d] - patch + 1, step) for d in range(nd)]
    import itertools
    if route == "gpu":
        g = PatchPoolFn.apply(x, patch, pool_out)
        g = g.reshape((-1,) + tuple(g.shape[2:]))
        for l in layers:
            g = conv(g, l.weight, l.bias)
        return g
    if route == "fused":
        if x.dtype != torch.float32:
            raise ValueError(f"patch_heads: the fused route takes an fp32 map, got {x.dtype}")
        return PatchHeadFn.apply(x, patch, pool_out, *_fused_params(layers, nd))
    if route != "torch":
        raise ValueError(f"patch_heads: route is 'torch', 'gpu' or 'fused', got {route!r}")
    if patch % pool_out == 0 and step % (patch // pool_out) == 0:
        w = patch // pool_out
        crop = tuple(slice(0, (x.shape[2 + d] // w) * w) for d in range(nd))
        g = (F.avg_pool2d if nd == 2 else F.avg_pool3d)(x[(slice(None), slice(None)) + crop], w)
        for l in layers:
            g = conv(g, l.weight, l.bias)
        return [g[(slice(None), slice(None)) + tuple(slice(o // w, o // w + pool_out) for o in org)]
                for org in itertools.product(*starts)]
    out = []
    pool = F.adaptive_avg_pool2d if nd == 2 else F.adaptive_avg_pool3d
    for org in itertools.product(*starts):
        y = pool(x[(slice(None), slice(None)) + tuple(slice(o, o + patch) for o in org)], pool_out)
        for l in layers:
            y = conv(y, l.weight, l.bias)
        out.append(y)
    return out


def mlp(head, x):
    """MLP.forward / MLP_3d.forward (model_2D.py:105-112): global average pooling, two linear layers."""
    m = _unwrap(head)
    y = m.gap(x).reshape(x.shape[0], -1)
    return F.linear(F.linear(y, m.f1.weight, m.f1.bias), m.f2.weight, m.f2.bias)


class QueueKLDFn(torch.autograd.Function):
    """F.kl_div(F.log_softmax(cs / Ts, 1), F.softmax(ct / Tt, 1), 'batchmean') of two fp32 matrices of raw cosines [N, L] as two kernels
    (csrc/queue_kld.hip): the forward reads each matrix once and keeps the per-row statistics [N, 3] float64, the backward is
    elementwise and writes each gradient OVER its cosine matrix - cs and ct are spent by it, the caller hands over matrices nobody else
    reads (queue_kld's GEMM outputs), and a second backward through the same node raises.  The gradient of a side that needs none (a
    detached teacher) is not computed."""

    @staticmethod
    def forward(ctx, cs, ct, Ts, Tt):
        from . import _lib as L
        L.require_gpu(cs, ct)
        if cs.dtype != torch.float32 or ct.dtype != torch.float32 or cs.dim() != 2 or cs.shape != ct.shape or cs.numel() == 0:
            raise ValueError(f"QueueKLDFn: two fp32 matrices [N, L] of one shape, got {cs.dtype} {tuple(cs.shape)} and {ct.dtype} {tuple(ct.shape)}")
        if not (Ts > 0 and Tt > 0):
            raise ValueError(f"QueueKLDFn: positive temperatures, got {Ts} and {Tt}")
        cs, ct = cs.contiguous(), ct.contiguous()
        N, Lq = cs.shape
        stats = torch.empty((N, 3), dtype=torch.float64, device=cs.device)
        loss = torch.empty((), dtype=torch.float32, device=cs.device)
        ctx.args = (N, Lq, Lq, Lq, 1.0 / Ts, 1.0 / Tt)
        L.call("arco_queue_kld_fwd", L.ptr(cs), L.ptr(ct), *ctx.args, L.ptr(stats), L.ptr(loss))
        ctx.save_for_backward(cs, ct, stats)
        ctx.spent = False
        return loss

    @staticmethod
    def backward(ctx, g):
        from . import _lib as L
        if ctx.spent:
            raise RuntimeError("QueueKLDFn: the first backward wrote the gradients over the cosine matrices; a second one through the same "
                               "graph has nothing to read")
        cs, ct, stats = ctx.saved_tensors
        need_s, need_t = ctx.needs_input_grad[:2]
        if not (need_s or need_t):
            return None, None, None, None
        ctx.spent = True
        Lq = ctx.args[1]
        g = g.detach().to(torch.float32).contiguous()
        L.call("arco_queue_kld_bwd", L.ptr(cs), L.ptr(ct), *ctx.args, L.ptr(stats), L.ptr(g),
               L.ptr(cs) if need_s else None, Lq, L.ptr(ct) if need_t else None, Lq)
        return cs.detach() if need_s else None, ct.detach() if need_t else None, None, None


KLD_ROUTES = ("torch", "fused")


def queue_kld(z_student, z_teacher, queue, Ts, Tt, route="torch"):
    """One KL-divergence-to-queue term of stage 1 (pretrain_2D.py:235-252): the batch-mean KL(softmax(teacher logits) || softmax(student
    logits)) of the rows of z_student and z_teacher against the rows of the queue snapshot.
    route="torch": KLD()(compute_logits(z_student, queue, Ts), compute_logits(z_teacher, queue, Tt)), literally.
    route="fused": the queue normalised once for both sides, the two cosine GEMMs by torch.matmul without a temperature, softmax,
    log-softmax, the pointwise KL, its sum and all their backwards in QueueKLDFn's two kernels.  The rows are normalised with autograd and
    the GEMM's backward carries the cosine gradients on, as on the torch route."""
    if route not in KLD_ROUTES:
        raise ValueError(f"queue_kld: route is 'torch' or 'fused', got {route!r}")
    if route == "torch":
        from .pretrain_2D import KLD
        return KLD()(compute_logits(z_student, queue, Ts), compute_logits(z_teacher, queue, Tt))
    qn_t = nn.functional.normalize(queue, dim=1).T
    cs = torch.matmul(nn.functional.normalize(z_student, dim=1), qn_t)
    ct = torch.matmul(nn.functional.normalize(z_teacher, dim=1), qn_t)
    return QueueKLDFn.apply(cs, ct, float(Ts), float(Tt))


def isd_embeddings(isd, im_q, im_k):
    """The training-mode forward up to the embeddings, before any logits: (outputs, ema_output_tmp, lat_q, lat_k, stu, tea, tea_tmp, queue,
    queue_mask) - the student's and the first teacher pass's segmentation outputs, the latent rows [B, F] of student and teacher, the
    patch-wise output rows [n, P] of both, the teacher's rows in the layout the mask queue stores, and the snapshots of the two queues,
    taken before the enqueue.  The reshapes are the reference's, view for view (they interleave patch and batch indices; the queues are
    stored in the layout they produce).  The KEY heads are not under no_grad in the reference (:268,282): they are EMA-updated and, being
    part of the KLD targets' graph, trained by the optimizer too."""
    batch_size = im_q.shape[0]
    outputs, latent_vector, _ = isd.model(im_q)
    with torch.no_grad():
        ema_output_tmp, _, _ = isd.ema_model(im_k)
        isd._momentum_update_key_encoder()
        shuffle_ids, reverse_ids = get_shuffle_ids(im_k.shape[0], im_k.device)          # ShuffleBN
        ema_output, ema_latent_vector, _ = isd.ema_model(im_k[shuffle_ids])
        ema_latent_vector = ema_latent_vector[reverse_ids]
        ema_output = ema_output[reverse_ids]
    queue = isd.queue.clone().detach()
    queue_mask = isd.queue_mask.clone().detach().transpose(0, 1).contiguous()
    route = getattr(isd, "patch_heads", "torch")
    stu = patch_heads(outputs, isd.patch_size, isd.q_outputs_head, isd.outputs_predictor, route)
    tea = patch_heads(ema_output, isd.patch_size, isd.k_outputs_head, None, route)
    stu = stu if torch.is_tensor(stu) else torch.cat(stu)          # the routes "gpu" and "fused" return the patches stacked already
    tea = tea if torch.is_tensor(tea) else torch.cat(tea)
    shp = tuple(stu.shape[1:])
    stu = stu.reshape(batch_size, -1, *shp).contiguous()
    tea = tea.reshape(batch_size, -1, *shp).contiguous()
    lat_k = mlp(isd.k_latent_head, ema_latent_vector)
    lat_q = mlp(isd.q_latent_head, latent_vector)
    for l in _unwrap(isd.latent_predictor):
        lat_q = F.linear(lat_q, l.weight, l.bias)
    tea_tmp = tea.reshape(tea.shape[0], tea.shape[1], -1).contiguous()
    stu = stu.reshape((stu.shape[1], batch_size, -1)).contiguous()
    tea = tea.reshape((tea.shape[1], batch_size, -1)).contiguous()
    stu = stu.reshape(-1, stu.shape[0]).contiguous()
    tea = tea.reshape(-1, tea.shape[0]).contiguous()
    queue_mask = queue_mask.reshape(-1, queue_mask.shape[0]).contiguous()
    return outputs, ema_output_tmp, lat_q, lat_k, stu, tea, tea_tmp, queue, queue_mask


def isd_enqueue(isd, lat_k, tea_tmp):
    with torch.no_grad():
        dequeue_and_enqueue(isd.K, lat_k, isd.queue, isd.queue_ptr)
        dequeue_and_enqueue(isd.K, tea_tmp, isd.queue_mask, isd.mask_queue_ptr)


def isd_forward(isd, im_q, im_k=None, Ts=None, Tt=None):
    """Returns (outputs, ema_output, ema_latent_logits, latent_logits, ema_output_logits, output_logits) in training mode,
    (outputs, latent) in eval mode; see isd_embeddings.  The logits are true logits whatever isd.kld says: the steppers take that route
    through isd_kld_terms, which builds none."""
    Ts = Ts if Ts else isd.Ts
    Tt = Tt if Tt else isd.Tt
    if not isd.training:
        outputs, latent_vector, _ = isd.model(im_q)
        return outputs, latent_vector
    outputs, ema_output_tmp, lat_q, lat_k, stu, tea, tea_tmp, queue, queue_mask = isd_embeddings(isd, im_q, im_k)
    ema_latent_logits = compute_logits(lat_k, queue, Tt)
    latent_logits = compute_logits(lat_q, queue, Ts)
    ema_output_logits = compute_logits(tea, queue_mask, Tt)
    output_logits = compute_logits(stu, queue_mask, Ts)
    isd_enqueue(isd, lat_k, tea_tmp)
    return outputs, ema_output_tmp, ema_latent_logits, latent_logits, ema_output_logits, output_logits


def isd_kld_terms(isd, im_q, im_k, Ts=None, Tt=None):
    """The training-mode forward for a stepper on a kld route that builds no logits: (outputs, ema_output, loss_latent, loss_output) with
    the two terms from queue_kld(route=isd.kld).  Generator consumption, queue snapshots and the enqueue are isd_forward's."""
    route = getattr(isd, "kld", "torch")
    if route not in KLD_ROUTES:
        raise ValueError(f"kld is 'torch' or 'fused', got {route!r}")
    Ts = Ts if Ts else isd.Ts
    Tt = Tt if Tt else isd.Tt
    outputs, ema_output_tmp, lat_q, lat_k, stu, tea, tea_tmp, queue, queue_mask = isd_embeddings(isd, im_q, im_k)
    loss_latent = queue_kld(lat_q, lat_k, queue, Ts, Tt, route)
    loss_output = queue_kld(stu, tea, queue_mask, Ts, Tt, route)
    isd_enqueue(isd, lat_k, tea_tmp)
    return outputs, ema_output_tmp, loss_latent, loss_output
