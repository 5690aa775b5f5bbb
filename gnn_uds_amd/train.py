"""The training and event-emulation loops of the reference's `surrogate/main.py` on device-resident data (`data.py`).

`fit` restates `main.py:209-239`: per epoch ONE random batch of windows -> `fit_eval(fit=True)` (-> `fit_grad_norm`), one test batch
-> `fit_eval(fit=False)`, a checkpoint every `save_gap` epochs.  The batch is drawn and built on the device (`WindowTable.draw`,
`WindowStore.batch`), losses stay device tensors until the end, so after epoch 0 the loop itself reads nothing back and uploads
nothing (`fit_eval`'s own finite test is unchanged).  `emulate_event` restates the `--test` loop (`main.py:327-362`): every sliding
window of one event through `Emulator.simulate`.  The reference's logging, TensorBoard scalars and best-model snapshots
(`main.py:234-261`) are the caller's business: the returned losses carry what they need.
"""
import torch


def _step(emul, table, batch_size, fit, bufs, ini):
    """One batch of `table` through fit_eval; bufs = [starts, batch tuple] of the previous epoch, filled again."""
    bufs[0] = table.draw(batch_size, out=bufs[0])
    bufs[1] = table.store.batch(bufs[0], out=bufs[1])
    losses = emul.fit_eval(*bufs[1], fit=fit)
    if fit and emul.gradnorm:
        if not ini:
            ini.extend(float(v) for v in losses)        # the first epoch's losses (main.py: `ini_loss`): the loop's one host read
        emul.fit_grad_norm(*bufs[1], ini)
    return torch.stack([v.reshape(()) for v in losses])


def fit(emul, train, test=None, epochs=1, batch_size=32, save_gap=None, model_dir=None):
    """Train `emul` for `epochs` epochs of one batch each from the `WindowTable` `train` (and evaluate one batch of `test` per epoch).
    Returns {'train_loss': (epochs, k), 'test_loss': (epochs, k) or None}: `fit_eval`'s [node, (flood,) edge] losses per epoch, device
    tensors.  Works with `emul.graphed_fit` on or off; the tables must sit on the model's device (`draw` is device only)."""
    for t in (train, test):
        if t is not None and (t.store.seq_in, t.store.seq_out, t.store.roll, bool(t.store.if_flood)) != (emul.seq_in, emul.seq_out, emul.roll,
                                                                                                      bool(emul.if_flood)):
            raise ValueError('the table\'s store cuts windows for (seq_in, seq_out, roll, if_flood) = %r, the model has %r'
                             % ((t.store.seq_in, t.store.seq_out, t.store.roll, t.store.if_flood), (emul.seq_in, emul.seq_out, emul.roll, emul.if_flood)))
    if save_gap and model_dir is None and emul.model_dir is None:
        raise ValueError('save_gap=%r needs a model_dir (or args.model_dir): there is nowhere to save to' % (save_gap,))
    train_loss, test_loss, ini = [], [], []
    train_bufs, test_bufs = [None, None], [None, None]
    for epoch in range(int(epochs)):
        train_loss.append(_step(emul, train, batch_size, True, train_bufs, ini))
        if test is not None:
            test_loss.append(_step(emul, test, batch_size, False, test_bufs, ini))
        if save_gap and (epoch + 1) % save_gap == 0:
            emul.save(model_dir)
    stack = lambda rows: torch.stack(rows) if rows else None
    return {'train_loss': stack(train_loss), 'test_loss': stack(test_loss)}


def emulate_event(emul, store, k, chunk=None):
    """Every sliding window of event `k` (interval 1, seq_out output rows) through `Emulator.simulate`, raw values in, `chunk`
    windows per call (None: all at once).  Returns (y_pred, ey_pred, y_true, ey_true); the truths are the raw Y / EY of the same
    windows."""
    starts = store.event_windows(k)
    n = starts.shape[0]
    if n == 0:
        raise ValueError('event %d (%d rows) is shorter than one window (%d + %d rows)' % (k, store.event_len[k], store.seq_in, store.seq_out))
    chunk = n if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError('chunk=%d' % chunk)
    parts = []
    with torch.no_grad():
        for lo in range(0, n, chunk):
            x, a, b, y, ex, ey = store.batch(starts[lo:lo + chunk], normalized=False, t_out=store.seq_out)
            y_pred, ey_pred = emul.simulate(x, b, a, ex)
            parts.append((y_pred, ey_pred, y, ey))
    return tuple(torch.cat(col, dim=0) for col in zip(*parts))
