"""LPIPS validation metric (net-lin / squeeze / v0.1) on the MI355X engine -- mirrors codes/models/modules/LPIPS."""
