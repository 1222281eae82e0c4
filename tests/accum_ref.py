"""Gradient accumulation restated in float64 (Lightning's accumulate_grad_batches = n, automatic
optimization): the n micro-batch gradients of a window are summed and divided by n, the mean is clipped
(optionally: by its 2-norm as torch.nn.utils.clip_grad_norm_, or by value), and one torch.optim.AdamW /
torch.optim.SGD-with-momentum update is made from it.  ``steps`` counts windows, so AdamW's bias
corrections do.  Flat tensors only; nothing here touches a device."""
import torch


class AccumRef:
    def __init__(self, which, p0, n, lr, weight_decay, betas=(0.9, 0.999), eps=1e-8, momentum=0.0,
                 clip_val=None, clip_algorithm="norm"):
        assert which in ("adamw", "sgd") and n >= 1
        self.which, self.n = which, n
        self.lr, self.wd, self.betas, self.eps, self.momentum = lr, weight_decay, betas, eps, momentum
        self.clip_val, self.clip_algorithm = clip_val, clip_algorithm
        self.p = p0.detach().double().reshape(-1).clone()
        self.exp_avg = torch.zeros_like(self.p)
        self.exp_avg_sq = torch.zeros_like(self.p)
        self.momentum_buf = torch.zeros_like(self.p)
        self.sum = torch.zeros_like(self.p)
        self.micro = 0
        self.steps = 0
        self.grad_norm = None      # of the last closed window's mean gradient, before clipping
        self.clip_coef = None

    def moments(self):
        if self.which == "adamw":
            return {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq}
        return {"momentum_buf": self.momentum_buf}

    def clipped_mean(self, total):
        g = total / self.n
        if self.clip_val:
            if self.clip_algorithm == "norm":
                self.grad_norm = float(g.square().sum().sqrt())
                self.clip_coef = min(1.0, self.clip_val / (self.grad_norm + 1e-6))
                g = g * self.clip_coef
            else:
                g = g.clamp(-self.clip_val, self.clip_val)
        return g

    def update(self, g):
        """One torch.optim.AdamW / SGD step from the gradient g."""
        self.steps += 1
        if self.which == "adamw":
            b1, b2 = self.betas
            self.p = self.p * (1.0 - self.lr * self.wd)
            self.exp_avg = b1 * self.exp_avg + (1.0 - b1) * g
            self.exp_avg_sq = b2 * self.exp_avg_sq + (1.0 - b2) * g * g
            bc1 = 1.0 - b1 ** self.steps
            bc2 = 1.0 - b2 ** self.steps
            denom = self.exp_avg_sq.sqrt() / bc2 ** 0.5 + self.eps
            self.p = self.p - (self.lr / bc1) * self.exp_avg / denom
        else:
            g = g + self.wd * self.p
            self.momentum_buf = g.clone() if self.steps == 1 else self.momentum * self.momentum_buf + g
            self.p = self.p - self.lr * (self.momentum_buf if self.momentum else g)

    def micro_step(self, grad):
        """Add one micro-batch gradient and make the optimizer call that follows it.  True when that
        call closed the window (and so updated)."""
        self.sum = self.sum + grad.detach().double().reshape(-1).cpu()
        self.micro += 1
        if self.micro < self.n:
            return False
        self.update(self.clipped_mean(self.sum))
        self.sum = torch.zeros_like(self.p)
        self.micro = 0
        return True
