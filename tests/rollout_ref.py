"""Rollout collection on the host: numpy twins of vpt_rollout_record_kernel (a scatter into column t) and vpt_rollout_reward_kernel (the per-environment
episode accumulators: float32, one add per step, so the GPU result equals it bit for bit), the chunk slicing of vpt_amd.rollout, a naive per-episode loop the
accumulator walk is checked against, and the scripted B = 3, T = 7 case both test files use.  A plain helper (no test, no fixture): numpy only, nothing of
vpt_amd."""
import numpy as np

F = np.float32


def record(bufs, t, img, first, act_buttons, act_camera, log_prob, vpred):
    """Column t of every buffer takes step t's values, in place; nan_flag [1] becomes 1 when a log-prob is NaN and is never cleared.
    bufs: dict(img [B, T, ...] uint8, first [B, T] uint8, act_buttons / act_camera [B, T] int64, old_log_prob / vpred [B, T] float32, nan_flag [1] uint8)."""
    b, t_len = bufs["first"].shape
    if not 0 <= t < t_len:
        raise ValueError(f"t = {t} is outside [0, {t_len})")
    lp = np.asarray(log_prob, F).reshape(b)
    bufs["img"][:, t] = np.asarray(img, np.uint8)
    bufs["first"][:, t] = np.asarray(first).reshape(b) != 0
    bufs["act_buttons"][:, t] = np.asarray(act_buttons, np.int64).reshape(b)
    bufs["act_camera"][:, t] = np.asarray(act_camera, np.int64).reshape(b)
    bufs["old_log_prob"][:, t] = lp
    bufs["vpred"][:, t] = np.asarray(vpred, F).reshape(b)
    if np.isnan(lp).any():
        bufs["nan_flag"][0] = 1


def new_reward_bufs(b, t_len, ep_return=None, ep_length=None):
    return dict(reward=np.zeros((b, t_len), F), done_return=np.zeros((b, t_len), F), done_length=np.zeros((b, t_len), np.int32),
                ep_return=np.zeros(b, F) if ep_return is None else np.asarray(ep_return, F).copy(),
                ep_length=np.zeros(b, np.int32) if ep_length is None else np.asarray(ep_length, np.int32).copy())


def reward_step(bufs, t, reward, done):
    """The environment's answer to step t, in place: R = ep_return + r (ONE float32 add), n = ep_length + 1; where done, (R, n) go to column t and the
    accumulators to 0; elsewhere column t gets 0 and the accumulators keep (R, n)."""
    b, t_len = bufs["reward"].shape
    if not 0 <= t < t_len:
        raise ValueError(f"t = {t} is outside [0, {t_len})")
    r, done = np.asarray(reward, F).reshape(b), np.asarray(done).reshape(b) != 0
    ret = (bufs["ep_return"] + r).astype(F)
    n = (bufs["ep_length"] + 1).astype(np.int32)
    bufs["reward"][:, t] = r
    bufs["done_return"][:, t] = np.where(done, ret, F(0))
    bufs["done_length"][:, t] = np.where(done, n, 0)
    bufs["ep_return"][:] = np.where(done, F(0), ret)
    bufs["ep_length"][:] = np.where(done, 0, n)


def chunk_bounds(horizon, chunk_len):
    """[(k L, (k + 1) L)]; the horizon must be a positive multiple of the chunk length."""
    if horizon < 1 or chunk_len < 1 or horizon % chunk_len:
        raise ValueError(f"horizon {horizon} is no positive multiple of chunk length {chunk_len}")
    return [(k * chunk_len, (k + 1) * chunk_len) for k in range(horizon // chunk_len)]


def chunk(arrays, k, chunk_len):
    """Chunk k of every [B, T, ...] array of a dict."""
    return {name: a[:, k * chunk_len:(k + 1) * chunk_len] for name, a in arrays.items()}


def episodes_naive(reward, done, ep_return0, ep_length0):
    """Per environment, episode by episode: the rewards of an episode collected in a list and added left to right in float32, starting from the return the
    episode brought along from the previous rollout.  -> (finished: list per environment of (step it ended at, return, length), open: per environment the
    (return, length) of the episode still running after the last step)."""
    b, t_len = np.asarray(reward).shape
    finished, running = [], []
    for i in range(b):
        eps, cur, carried, n0 = [], [], F(ep_return0[i]), int(ep_length0[i])
        for t in range(t_len):
            cur.append(F(reward[i][t]))
            if done[i][t]:
                total = carried
                for x in cur:
                    total = F(total + x)
                eps.append((t, total, n0 + len(cur)))
                cur, carried, n0 = [], F(0), 0
        total = carried
        for x in cur:
            total = F(total + x)
        finished.append(eps)
        running.append((total, n0 + len(cur)))
    return finished, running


def scripted_case():
    """B = 3, T = 7.  Environment 0: an episode ends at step 0 (it continues from a previous rollout: incoming return 2.5 over 4 steps), two more end on the
    consecutive steps 3 and 4, and one ends at the last step.  Environment 1 never finishes.  Environment 2: ends at steps 1 and 2 (consecutive), comes
    in with a non-zero return, and is still running at the end.  The rewards mix 2^24, 1 and -2^24: (2^24 + 1) - 2^24 is 0 in float32 and 1 when the
    adds are re-associated, so any kernel that sums in another order is caught."""
    big = F(2.0 ** 24)
    reward = np.array([[1.0, big, 1.0, -big, 0.25, 0.1, 0.2],
                       [big, 1.0, 1.0, -big, 0.3, 1e-3, 7.0],
                       [0.5, 0.75, -1.5, 1.0, big, 1.0, -big]], F)
    done = np.array([[1, 0, 0, 1, 1, 0, 1],
                     [0, 0, 0, 0, 0, 0, 0],
                     [0, 1, 1, 0, 0, 0, 0]], bool)
    ep_return0, ep_length0 = np.array([2.5, 0.0, -0.125], F), np.array([4, 0, 2], np.int32)
    return reward, done, ep_return0, ep_length0
