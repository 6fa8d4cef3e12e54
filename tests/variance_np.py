"""The measured variance of include/hrt.h ("measured variance") restated in numpy float32 from the header's words: the same
operations in the same order, one IEEE fp32 rounding each, vectorised over the pixels.  It shares nothing with csrc/hrt_variance.hip;
tests/test_gpu_variance.py requires the kernels to give its bits, tests/test_variance_cpu.py checks its properties and decides the quality
test on it."""
import numpy as np

F = np.float32


def lum(r, g, b):
    return F(0.2126) * r + F(0.7152) * g + F(0.0722) * b


def _pos(x):
    """max(0, x) of the header: x > 0 ? x : 0"""
    return np.where(x > 0, x, F(0)).astype(F)


def fold(rgb, scale, done, c, state=None):
    """One fold: rgb [..., 3] the accumulation buffer after a batch of c samples that follows `done` earlier ones, state [..., 2] =
    (yprev, M2) (ignored when done == 0) -> the new state [..., 2]."""
    rgb = np.asarray(rgb, F)
    with np.errstate(all="ignore"):
        y = lum(rgb[..., 0], rgb[..., 1], rgb[..., 2]) * F(scale)
        if done == 0:
            m2 = np.zeros_like(y)
        else:
            state = np.asarray(state, F)
            yprev, m2_old = state[..., 0], state[..., 1]
            mb = (y - yprev) / F(c)
            mp = yprev / F(done)
            d = mb - mp
            w = (F(done) * F(c)) / F(done + c)
            m2 = m2_old + (d * d) * w
    return np.stack([y, m2], axis=-1).astype(F)


def finish(state, samples, batches):
    """state [..., 2] after `batches` folds over `samples` samples -> the variance of the mean luminance [...]"""
    state = np.asarray(state, F)
    with np.errstate(all="ignore"):
        return (_pos(state[..., 1] / F(batches - 1)) / F(samples)).astype(F)


def adaptive(sums, sq, count):
    """The variance of the mean luminance from the buffers of an adaptive render; 0 where count < 2."""
    sums, sq = np.asarray(sums, F), np.asarray(sq, F)
    n = np.asarray(count).astype(F)
    with np.errstate(all="ignore"):
        m = lum(sums[..., 0], sums[..., 1], sums[..., 2]) / n
        v = _pos((sq - n * m * m) / (n - F(1))) / n
    return np.where(np.asarray(count) >= 2, v, F(0)).astype(F)


def batch_ranges(samples, batches):
    """The sample ranges of a render split into `batches` passes: range j starts at j * ceil(samples / batches), the last non-empty one
    takes what is left -> [(first, count), ...] (fewer than `batches` entries when the ranges run out first)."""
    step = -(-samples // batches)
    return [(s, min(step, samples - s)) for s in range(0, samples, step)]


def from_batches(buffers, counts, samples=None):
    """The whole pipeline over accumulation buffers: buffers[j] is the buffer after batch j of counts[j] samples; when `samples` is given
    the last one has been divided by it (scale = samples), otherwise every buffer holds undivided sums.  -> variance [...]"""
    done, state = 0, None
    for j, (buf, c) in enumerate(zip(buffers, counts)):
        last = j == len(counts) - 1
        state = fold(buf, F(samples) if (last and samples is not None) else F(1), done, c, state)
        done += c
    return finish(state, done, len(counts))
